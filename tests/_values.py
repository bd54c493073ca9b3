"""Block-value helpers shared by the tests that move values into a handle's packed image or read them out again
(update_blocks / refresh, device-resident blocks, the COO export).  Test code only; `torch` is passed in by the GPU
tests, so that this module imports without it."""
import ctypes as C

import numpy as np

from _common import BLOCK_KEYS as KEYS
from _gpu import dev_copy

MEM_HOST, MEM_DEVICE = 0, 1  # BSM_MEM_HOST / BSM_MEM_DEVICE


def src_list(p):
    return [b for k in KEYS if k in p and not (k == "blocks" and p["kind"] == "symmetric") for b in p[k]]


def with_values(p, vals):
    """problem p with its blocks (constructor order: blocks, or diagonals + offdiagonals) replaced by vals"""
    q = dict(p)
    if p["kind"] == "symmetric":
        nd = len(p["diagonals"])
        q["diagonals"], q["offdiagonals"] = list(vals[:nd]), list(vals[nd:])
    else:
        q["blocks"] = list(vals)
    return q


def on_device(torch, p):
    """the same problem with its blocks in HBM (column-major CUDA tensors): a handle built from it refills from
    device memory"""
    return with_values(p, [dev_copy(torch, b) for b in src_list(p)])


def new_values(p, rng):
    out = []
    for b in src_list(p):
        r = rng.standard_normal(b.shape)
        if np.iscomplexobj(b):
            r = r + 1j * rng.standard_normal(b.shape)
        out.append(np.asfortranarray(r.astype(b.dtype)))
    return out


def block_indices(p):
    """[(rows, cols)] of every block of p in constructor order (src_list's), 1-based"""
    if p["kind"] == "vbcrs":
        return [(np.arange(r0, r0 + b.shape[0]), np.arange(c0, c0 + b.shape[1]))
                for b, r0, c0 in zip(p["blocks"], p["rowstart"], p["colstart"])]
    pairs = [(np.asarray(r), np.asarray(c)) for r, c in zip(p["rowindices"], p["colindices"])]
    if p["kind"] == "symmetric":
        return [(np.asarray(d), np.asarray(d)) for d in p["diagonalindices"]] + pairs
    return pairs


def diagonal_shift(p, d):
    """the blocks of p + diag(d) that differ from p's -> (1-based ids in constructor order, their new values): entry (i, i)
    takes d[i] in the FIRST block that holds it (blocks may overlap: their values sum), every other block keeps its values
    and is not listed.  A square host problem whose every diagonal entry with d != 0 lies in some block, and for the
    symmetric kind in a diagonal block (a mirrored off-diagonal one would count it twice)"""
    src, idx = src_list(p), block_indices(p)
    nd = len(p["diagonals"]) if p["kind"] == "symmetric" else len(src)
    done = np.zeros(p["size"][0], dtype=bool)
    ids, out = [], []
    for k, (b, (r, c)) in enumerate(zip(src, idx)):
        a, q = np.nonzero(r[:, None] == c[None, :])
        take = ~done[r[a] - 1]
        if not take.any():
            continue
        assert k < nd, "a diagonal entry lies in an off-diagonal block only"
        new = np.array(b, order="F", copy=True)
        new[a[take], q[take]] += np.asarray(d)[r[a[take]] - 1].astype(b.dtype)
        done[r[a[take]] - 1] = True
        ids.append(k + 1)
        out.append(new)
    assert np.all(done | (np.asarray(d) == 0)), "a shifted diagonal entry lies in no block"
    return ids, out


def update_rc(A, ids, blocks, lds, memspace=MEM_HOST, stream=None, nupd=None):
    """bsm_update_blocks straight through the C ABI (1-based ids or None; numpy or CUDA-tensor blocks; nupd: the count
    passed in place of len(blocks)) -> its return code"""
    from bsm_amd import _lib as L
    I = C.POINTER(C.c_int64)
    idv = None if ids is None else np.ascontiguousarray(list(ids), dtype=np.int64)
    ptrs = (C.c_void_p * max(len(blocks), 1))(*[(b.data_ptr() if hasattr(b, "data_ptr") else b.ctypes.data) for b in blocks])
    ldv = np.ascontiguousarray(lds, dtype=np.int64)
    return L.lib().bsm_update_blocks(A._h.ptr, len(blocks) if nupd is None else nupd,
                                     None if idv is None else idv.ctypes.data_as(I), ptrs, ldv.ctypes.data_as(I), memspace, stream)


def raw_update(A, ids, blocks, lds, memspace, stream=None):
    """update_rc that raises on an error code"""
    from bsm_amd import _lib as L
    L.check(update_rc(A, ids, blocks, lds, memspace, stream))


def padded(torch, b, pad, device):
    """b inside a column-major array with ld = m + pad (host array or CUDA tensor); returns (array, ld)"""
    m, n = b.shape
    a = np.zeros((m + pad, n), dtype=b.dtype, order="F")
    a[:m] = b
    a[m:] = np.nan  # rows outside the block must never be read
    if device:
        return dev_copy(torch, a), m + pad
    return a, m + pad


# ---- the value fuzz (test_fuzz_values_cpu.py, test_gpu_fuzz_values.py) -------------------------------------------------
NOPS = 12  # operators per (kind, element type)
FEATURES = {"blocksparse": ("empty", "tall", "thin", "shared", "scattered"), "vbcrs": ("tall", "thin", "shared"),
            "symmetric": ("tall", "thin", "shared", "scattered")}
ACC = ("auto", "atomic", "gather")


def value_seed(kind, dtype):
    from _fuzz import seed_of
    return seed_of(kind, np.dtype(dtype)) + 7000


def value_operators(kind, dtype):
    """the NOPS operators of a (kind, element type): drawn first and in one go from the stream of value_seed, so the
    CPU and the GPU test see the same ones whatever else they draw (new values come from other generators)"""
    from _fuzz import GEN
    rng = np.random.default_rng(value_seed(kind, dtype))
    return [GEN[kind](rng, np.dtype(dtype)) for _ in range(NOPS)]


def options(kind, case):
    """constructor options of operator `case`: the accumulate modes in turn, a transposed image on every second
    block-sparse / VBCRS operator"""
    kw = {"accumulate": ACC[case % len(ACC)]}
    if kind != "symmetric" and case % 2 == 1:
        kw["transpose_image"] = True
    return kw


def assert_coverage(kind, dtype, problems):
    """every layout edge the kind can reach is reached by at least two of the operators"""
    from _fuzz import edge_features
    feats = [edge_features(p) for p in problems]
    count = {f: sum(f in s for s in feats) for f in FEATURES[kind]}
    assert all(c >= 2 for c in count.values()), (kind, np.dtype(dtype).name, count)
    return count


def copied(p):
    """p with its blocks copied: a mirror built from it may be edited in place without touching p"""
    return with_values(p, [np.array(b, order="F") for b in src_list(p)])


def nan_blocks(p):
    """p with every block full of NaN: a slot a later refill misses shows as NaN"""
    return with_values(p, [np.full(b.shape, np.nan, dtype=b.dtype, order="F") for b in src_list(p)])


# values that round differently under truncation than under round-to-nearest-even (ties to even below and above, just above
# a tie), values subnormal in single precision (kept; the tie 2^-150 rounds to zero) and beyond its range (+-inf; the last
# one is the tie between the largest float and 2^128)
SPECIAL = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -(1 + 2.0 ** -24 + 2.0 ** -40), 1e-40, -3e-42, 2.0 ** -149, 2.0 ** -150,
           1.5 * 2.0 ** -149, 1e39, -1e39, 2.0 ** 128 - 2.0 ** 103]


def seeded(p):
    """p (double or complex double) with SPECIAL written over the head of its largest block, column-major (complex: over
    the real parts, and in reverse over the imaginary parts)"""
    src = [np.array(b, order="F") for b in src_list(p)]
    b = max(src, key=lambda a: a.size)
    k = min(len(SPECIAL), b.size)
    assert k > 8  # up to the first value beyond the range of single precision
    flat = b.reshape(-1, order="F")
    assert np.shares_memory(flat, b)
    if b.dtype.kind == "c":
        flat[:k].real = SPECIAL[:k]
        flat[:k].imag = SPECIAL[:k][::-1]
    else:
        flat[:k] = SPECIAL[:k]
    return with_values(p, src)


def subset_of(rng, p, cur):
    """a random third of the block ids in random order with new values -> (ids, new blocks, values afterwards)"""
    nb = len(cur)
    ids = rng.permutation(nb)[: max(1, nb // 3)] + 1
    fresh = new_values(p, rng)
    out = list(cur)
    for i in ids:
        out[i - 1] = fresh[i - 1]
    return ids, [fresh[i - 1] for i in ids], out


def explain(p, seed, case, got, want):
    """assert message for two canonical triple arrays that differ: the first differing triple of each and the blocks of p
    that cover the expected one"""
    if got.shape != want.shape:
        head = f"{len(got)} triples, expected {len(want)}"
        n = min(len(got), len(want))
        bad = np.nonzero(np.any(got[:n] != want[:n], axis=1))[0]
        k = int(bad[0]) if len(bad) else n
    else:
        k = int(np.nonzero(np.any(got != want, axis=1))[0][0])
        head = f"{int(np.sum(np.any(got != want, axis=1)))} of {len(want)} triples differ"
    show = lambda t: None if t is None else (int(t[0] >> 32), int(t[0] & 0xffffffff)) + tuple(hex(v) for v in t[1:])  # noqa: E731
    g = got[k].tolist() if k < len(got) else None
    w = want[k].tolist() if k < len(want) else None
    where = covering_blocks(p, *show(w)[:2]) if w is not None else []
    return (f"seed {seed} case {case} ({p['kind']}): {head}; first at {k}: got (row, col, value bits) {show(g)}, "
            f"expected {show(w)}, in blocks {where}")


def covering_blocks(p, r, c):
    """1-based ids (constructor order) of the blocks of p that hold entry (r, c)"""
    out = []
    if p["kind"] == "vbcrs":
        for b, (blk, r0, c0) in enumerate(zip(p["blocks"], p["rowstart"], p["colstart"])):
            if r0 <= r < r0 + blk.shape[0] and c0 <= c < c0 + blk.shape[1]:
                out.append(b + 1)
    elif p["kind"] == "blocksparse":
        for b, (ri, ci) in enumerate(zip(p["rowindices"], p["colindices"])):
            if r in ri and c in ci:
                out.append(b + 1)
    else:
        nd = len(p["diagonals"])
        for b, d in enumerate(p["diagonalindices"]):
            if r in d and c in d:
                out.append(b + 1)
        for b, (ri, ci) in enumerate(zip(p["rowindices"], p["colindices"])):
            if (r in ri and c in ci) or (c in ri and r in ci):
                out.append(nd + b + 1)
    return out


def image_parts(A):
    """every array of the host image of an analysis-only handle as bytes: values / t_values are what a refill rewrites,
    the others are metadata"""
    from _common import get_image
    from bsm_amd import _lib as L
    out = {}
    for w in (0, 8):
        v, r, c, wv = get_image(A, timage=False, multi=(w == 8))
        if w == 0:
            out.update(values=v.tobytes(), rows=r.tobytes(), cols=c.tobytes(), waves=wv.tobytes())
        else:
            out["waves_multi"] = wv.tobytes()
    n = C.c_int64(0)
    if L.lib().bsm_get_image(A._h.ptr, 16, None, C.byref(n)) == 0:
        v, r, c, wv = get_image(A, timage=True)
        out.update(t_values=v.tobytes(), t_rows=r.tobytes(), t_cols=c.tobytes(), t_waves=wv.tobytes())
    return out
