"""Seeded random operators for the differential tests (CPU: packed-image interpreter vs oracle;
GPU: HIP path vs oracle).  The generator aims at the corners of the packed layout rather than at
realism: row counts around the 8/16/32/64 lane-group boundaries and the 64-row chunk limit, single
rows and columns, empty blocks, repeated row sets (merged panels), overlapping row ranges, unsorted
and strided index lists, rectangular operators, more than three column runs per panel.
For the multi-GPU layers: `squared`, the documented row partition in numpy (`partition_rule`) and the partition edges a
(problem, number of parts) pair reaches (`partition_features`).  Also what the fuzz suites share: the cross-type
pairs, `rounded` / `cast_blocks`, `build_fuzz` (the coloured-mode rule), the strict error norm `fuzz_err` and the `Stat`
counter behind the PAIRSTAT / DISTDEV lines."""
import numpy as np

from _common import BLOCK_KEYS

EDGE = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 129]


def _size(rng):
    return int(rng.choice(EDGE)) if rng.random() < 0.7 else int(rng.integers(1, 90))


def _block(rng, m, n, dtype):
    b = rng.standard_normal((m, n))
    if np.dtype(dtype).kind == "c":
        b = b + 1j * rng.standard_normal((m, n))
    return np.asfortranarray(b.astype(dtype))


def _index_list(rng, k, n):
    """k distinct 1-based indices: contiguous, strided, sorted-scattered or shuffled"""
    mode = rng.integers(0, 4)
    if mode == 0 or k == 1:
        s = int(rng.integers(1, n - k + 2))
        return np.arange(s, s + k, dtype=np.int64)
    if mode == 1 and 2 * k <= n:
        s = int(rng.integers(1, n - 2 * k + 2))
        return np.arange(s, s + 2 * k, 2, dtype=np.int64)
    idx = rng.choice(n, size=k, replace=False).astype(np.int64) + 1
    return np.sort(idx) if mode == 2 else idx


def random_blocksparse(rng, dtype, colourable=False):
    """colourable: the blocks of one row set take pairwise disjoint column lists (drawn among the columns the set does not
    hold yet), so that the coloured accumulation mode -- which refuses a row set that repeats a column index -- builds.
    The default draws exactly what it always drew: the operators of the existing seeds do not change."""
    nr, nc = int(rng.integers(150, 700)), int(rng.integers(150, 700))
    blocks, rows, cols = [], [], []
    pool = []  # row sets that get reused: several blocks on the SAME rows merge into one panel
    # colourable: the columns held already, per run of at most 64 rows of a row list -- the unit the analysis merges (two
    # different lists share a panel where such a run of theirs coincides, e.g. the first 64 of 100 and of 65 rows) -- and
    # the rows held per run of columns, for the transposed ordering of a handle built with transpose_image
    held, held_t = {}, {}
    none = np.zeros(0, np.int64)

    def runs_of(v):
        return [tuple(int(i) for i in v[a:a + 64]) for a in range(0, len(v), 64)]

    def columns(r, n):
        if not colourable:
            return _index_list(rng, n, nc) if n else none
        taken = [held[k] for k in runs_of(r) if k in held]
        free = np.setdiff1d(np.arange(1, nc + 1, dtype=np.int64), np.concatenate(taken) if taken else none)
        n = min(n, len(free))
        c = none
        for _ in range(8 if n else 0):  # (a clash in the transposed ordering needs an identical run of columns: rare)
            c = free[_index_list(rng, n, len(free)) - 1]
            if not any(k in held_t and len(np.intersect1d(held_t[k], r)) for k in runs_of(c)):
                break
            c = none
        if len(c) and len(r):
            for k in runs_of(r):
                held[k] = np.concatenate([held[k], c]) if k in held else c
            for k in runs_of(c):
                held_t[k] = np.concatenate([held_t[k], r]) if k in held_t else r
        return c

    for _ in range(int(rng.integers(1, 40))):
        if pool and rng.random() < 0.4:
            r = pool[int(rng.integers(0, len(pool)))]
        else:
            r = _index_list(rng, min(_size(rng), nr), nr)
            pool.append(r)
        n = 0 if rng.random() < 0.05 else min(_size(rng), nc)
        c = columns(r, n)
        if rng.random() < 0.05:
            r = np.zeros(0, np.int64)
        blocks.append(_block(rng, len(r), len(c), dtype))
        rows.append(r)
        cols.append(c)
    if rng.random() < 0.2:  # one very wide panel: many x chunks, a row group cut into several work items
        r = _index_list(rng, int(rng.choice([17, 40, 64])), nr)
        for _ in range(int(rng.integers(8, 30))):
            c = columns(r, min(int(rng.integers(60, 130)), nc))
            blocks.append(_block(rng, len(r), len(c), dtype))
            rows.append(r)
            cols.append(c)
    return dict(kind="blocksparse", blocks=blocks, rowindices=rows, colindices=cols, size=(nr, nc))


def random_vbcrs(rng, dtype):
    nr, nc = int(rng.integers(150, 900)), int(rng.integers(150, 900))
    blocks, r0, c0 = [], [], []
    starts = []
    for _ in range(int(rng.integers(1, 50))):
        m, n = min(_size(rng), nr), min(_size(rng), nc)
        if starts and rng.random() < 0.5:  # another block of an existing block row
            rs, m = starts[int(rng.integers(0, len(starts)))]
        else:
            rs = int(rng.integers(1, nr - m + 2))
            starts.append((rs, m))
        blocks.append(_block(rng, m, n, dtype))
        r0.append(rs)
        c0.append(int(rng.integers(1, nc - n + 2)))
    return dict(kind="vbcrs", blocks=blocks, rowstart=np.array(r0, np.int64), colstart=np.array(c0, np.int64),
                size=(nr, nc))


def random_symmetric(rng, dtype):
    n = int(rng.integers(200, 800))
    perm = rng.permutation(n) + 1 if rng.random() < 0.5 else np.arange(1, n + 1)
    sets, pos = [], 0
    while pos < n:
        k = min(_size(rng) if rng.random() < 0.5 else int(rng.integers(1, 40)), n - pos)
        s = perm[pos:pos + k].astype(np.int64)
        sets.append(np.sort(s) if rng.random() < 0.5 else s)
        pos += k
        if rng.random() < 0.1:
            pos += int(rng.integers(0, 20))  # rows no block covers
    diags, dsets = [], []
    for s in sets:
        if rng.random() < 0.85:
            d = _block(rng, len(s), len(s), dtype)
            diags.append(np.asfortranarray((d + d.T) / 2))
            dsets.append(s)
    offs, ri, ci = [], [], []
    for _ in range(int(rng.integers(0, 3 * len(sets)))):
        i, j = int(rng.integers(0, len(sets))), int(rng.integers(0, len(sets)))
        if i == j:
            continue
        offs.append(_block(rng, len(sets[i]), len(sets[j]), dtype))
        ri.append(sets[i])
        ci.append(sets[j])
    if rng.random() < 0.2 and len(sets) > 3:  # one row set coupled to (almost) every other: a very wide panel
        i = int(rng.integers(0, len(sets)))
        for j in range(len(sets)):
            if j != i and rng.random() < 0.9:
                offs.append(_block(rng, len(sets[i]), len(sets[j]), dtype))
                ri.append(sets[i])
                ci.append(sets[j])
    return dict(kind="symmetric", diagonals=diags, diagonalindices=dsets, offdiagonals=offs, rowindices=ri,
                colindices=ci, size=(n, n))


GEN = {"blocksparse": random_blocksparse, "vbcrs": random_vbcrs, "symmetric": random_symmetric}

# the cross-type pairs (block type of the operator, vector type, storage= of the constructor): mixed storage (values kept
# in single precision under double vectors) and real operators under complex vectors
CROSS_PAIRS = [(np.float64, np.float64, np.float32), (np.complex128, np.complex128, np.complex64),
               (np.float64, np.complex128, None), (np.float32, np.complex64, None)]


def rounded(problem, S):
    """the problem a mixed-storage handle holds: every block rounded once to the stored type S, back in double"""
    q = dict(problem)
    for k in BLOCK_KEYS:
        if k in problem:
            q[k] = [np.asfortranarray(b.astype(S).astype(np.result_type(S, np.float64))) for b in problem[k]]
    return q


def cast_blocks(problem, dtype):
    q = dict(problem)
    for k in BLOCK_KEYS:
        if k in problem:
            q[k] = [np.asfortranarray(b.astype(dtype)) for b in problem[k]]
    return q


def restrict_rows(problem, lo, hi):
    """The blocks whose rows all lie in lo .. hi (1-based, inclusive): the operator a handle built with own=(lo, hi) may
    hold if no row outside the range is to be touched.  An off-diagonal block of a symmetric operator reaches the rows of
    its column list too (its transposed half), so both lists must lie inside."""
    inside = lambda idx: bool(np.all((np.asarray(idx) >= lo) & (np.asarray(idx) <= hi)))  # noqa: E731
    q = dict(problem)
    k = problem["kind"]
    if k == "blocksparse":
        keep = [b for b, r in enumerate(problem["rowindices"]) if inside(r)]
        q.update(blocks=[problem["blocks"][b] for b in keep], rowindices=[problem["rowindices"][b] for b in keep],
                 colindices=[problem["colindices"][b] for b in keep])
    elif k == "vbcrs":
        keep = [b for b, (r, blk) in enumerate(zip(problem["rowstart"], problem["blocks"]))
                if r >= lo and r + blk.shape[0] - 1 <= hi]
        q.update(blocks=[problem["blocks"][b] for b in keep], rowstart=problem["rowstart"][keep],
                 colstart=problem["colstart"][keep])
    else:
        kd = [b for b, d in enumerate(problem["diagonalindices"]) if inside(d)]
        ko = [b for b, (r, c) in enumerate(zip(problem["rowindices"], problem["colindices"])) if inside(r) and inside(c)]
        q.update(diagonals=[problem["diagonals"][b] for b in kd], diagonalindices=[problem["diagonalindices"][b] for b in kd],
                 offdiagonals=[problem["offdiagonals"][b] for b in ko], rowindices=[problem["rowindices"][b] for b in ko],
                 colindices=[problem["colindices"][b] for b in ko])
    return q


def build_fuzz(bsm, rng, kind, dtype, acc, redraws=5, **kw):
    """One operator of GEN[kind] and its handle in accumulation mode acc -> (problem, handle), (problem, None) when the
    analysis refuses the coloured mode.  The rule of the cross-pair tests for the coloured mode: block-sparse operators are
    drawn colourable and always build; a symmetric operator whose row groups repeat a column index (one pair of row sets
    drawn twice) is redrawn, up to `redraws` times; every other refusal is an error."""
    colored = acc == "colored"
    for _ in range(redraws + 1 if colored and kind == "symmetric" else 1):
        p = random_blocksparse(rng, dtype, colourable=True) if colored and kind == "blocksparse" else GEN[kind](rng, dtype)
        try:
            return p, bsm.synthetic.build(p, accumulate=acc, **kw)
        except RuntimeError as e:
            assert colored and kind == "symmetric" and "repeat" in str(e), (kind, acc, str(e))
    return p, None


def fuzz_err(got, ref):
    """max|got - ref| / max|ref|, the norm of the fuzz suites.  Unlike _common.relerr an all-zero reference does not
    divide by 1 but by 1e-30: any non-zero entry of `got` then fails"""
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-30)) if len(ref) else 0.0


def scalar_sets(dt):
    """(alpha, beta, strong zero) of the one-column legs of the GPU fuzz suites; complex vectors add a complex pair"""
    s = [(1, 0, True), (-0.5, 1.25, False)]
    return s + [(0.5 - 0.25j, 1.5 + 0.5j, False)] if np.dtype(dt).kind == "c" else s


class Stat:
    """The counters of one GPU fuzz test: every check prints its error and feeds `worst`; `done` prints the summary line
    docs/ quote and asserts that at least half of the coloured cases ran."""

    def __init__(self, *tag):
        self.tag, self.worst = tag, 0.0
        self.products = self.columns = self.cases = self.empty_parts = self.coloured = self.ran = 0

    def check(self, got, ref, tol, what):
        e = fuzz_err(got, ref)
        print(f"  {self.tag} {what}: {e:.3e}")
        self.worst = max(self.worst, e) if e == e else float("nan")
        self.columns += 1
        assert e < tol, (self.tag, what, e)

    def done(self, head, counts):
        print("{} {} {} {} worst {:.3e} {} coloured {} of {}".format(head, *self.tag, self.worst, counts, self.ran, self.coloured))
        assert 2 * self.ran >= self.coloured, (self.tag, self.ran, self.coloured)


# ---- the entries of an operator, straight from its numpy blocks (no library code) --------------------------------------
def coo_triples(problem):
    """(rows, cols, vals), 1-based: every entry of every block, the off-diagonal blocks of a symmetric operator a second
    time transposed (not conjugated); overlapping blocks give one triple each, empty blocks none"""
    rows, cols, vals = [], [], []

    def push(b, ri, ci):
        b = np.asarray(b)
        if b.size == 0:
            return
        ri, ci = np.asarray(ri, dtype=np.int64), np.asarray(ci, dtype=np.int64)
        rows.append(np.repeat(ri, len(ci)))  # row-major enumeration of the block
        cols.append(np.tile(ci, len(ri)))
        vals.append(np.ascontiguousarray(b).ravel())

    k = problem["kind"]
    if k == "vbcrs":
        for b, r0, c0 in zip(problem["blocks"], problem["rowstart"], problem["colstart"]):
            push(b, int(r0) + np.arange(b.shape[0]), int(c0) + np.arange(b.shape[1]))
    elif k == "blocksparse":
        for b, r, c in zip(problem["blocks"], problem["rowindices"], problem["colindices"]):
            push(b, r, c)
    else:
        for b, d in zip(problem["diagonals"], problem["diagonalindices"]):
            push(b, d, d)
        for b, r, c in zip(problem["offdiagonals"], problem["rowindices"], problem["colindices"]):
            push(b, r, c)
            push(np.asarray(b).T, c, r)
    if not rows:
        first = [b for key in BLOCK_KEYS for b in problem.get(key, [])]
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, first[0].dtype if first else np.float64)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def canonical(rows, cols, vals):
    """The triples sorted by (row, col, bit pattern of the value) as one uint64 array with a row per triple: row << 32 | col,
    then the value's bytes as unsigned integers (real part, imaginary part).  Duplicate positions of overlapping blocks,
    NaNs and signed zeros compare exactly: two sets of triples are equal when their canonical forms are array_equal."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    vals = np.ascontiguousarray(vals)
    assert rows.shape == cols.shape == vals.shape and rows.ndim == 1
    assert len(rows) == 0 or (rows.min() >= 0 and cols.min() >= 0 and rows.max() < 2 ** 31 and cols.max() < 2 ** 32), \
        ("an index outside 0 .. 2^31", int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max()))
    word = {4: np.uint32, 8: np.uint64}[vals.dtype.itemsize // (2 if vals.dtype.kind == "c" else 1)]
    bits = vals.view(word).reshape(len(vals), 2 if vals.dtype.kind == "c" else 1).astype(np.uint64)
    out = np.empty((len(vals), 1 + bits.shape[1]), dtype=np.uint64)
    out[:, 0] = (rows.astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    out[:, 1:] = bits
    order = np.lexsort(tuple(out[:, k] for k in range(out.shape[1] - 1, -1, -1)))
    return out[order]


def edge_features(problem):
    """which of the layout edges the operator reaches: "empty" (a block of size 0), "tall" (a block of more than 64 rows:
    several chunks), "thin" (a non-empty block of one row or one column), "shared" (a row list / row start that two or more
    blocks use: a merged panel), "scattered" (an index list that is not contiguous)"""
    k = problem["kind"]
    blocks = [b for key in BLOCK_KEYS for b in problem.get(key, [])]
    out = set()
    if any(b.size == 0 for b in blocks):
        out.add("empty")
    if any(b.shape[0] > 64 for b in blocks):
        out.add("tall")
    if any(b.size > 0 and 1 in b.shape for b in blocks):
        out.add("thin")
    if k == "vbcrs":
        rowkeys, lists = [int(r) for r in problem["rowstart"]], []
    else:
        rlists = list(problem.get("diagonalindices", [])) + list(problem["rowindices"])
        rowkeys = [tuple(int(i) for i in r) for r in rlists if len(r)]
        lists = rlists + list(problem["colindices"])
    if len(set(rowkeys)) < len(rowkeys):
        out.add("shared")
    if any(len(v) > 1 and np.any(np.diff(np.asarray(v)) != 1) for v in lists):
        out.add("scattered")
    return out


def squared(problem):
    """the same blocks with size = (n, n), n = max(size): rows and columns can then be partitioned alike (the
    partitioned-vector legs of the multi-GPU layers on block-sparse and VBCRS operators); symmetric operators come back
    as they are"""
    q = dict(problem)
    n = int(max(problem["size"]))
    q["size"] = (n, n)
    return q


def block_lists(problem):
    """per block, in the order the multi-GPU layers number them (symmetric: diagonals first) -> (row hulls, column hulls,
    row keys, weights); a hull is (lo, hi) 1-based inclusive or None for an empty list, the key of a block is its smallest
    row index (1 for an empty list), its weight the stored entries"""
    k = problem["kind"]
    if k == "vbcrs":
        rl = [np.arange(int(r), int(r) + b.shape[0]) for r, b in zip(problem["rowstart"], problem["blocks"])]
        cl = [np.arange(int(c), int(c) + b.shape[1]) for c, b in zip(problem["colstart"], problem["blocks"])]
        blocks = problem["blocks"]
    elif k == "blocksparse":
        rl, cl, blocks = list(problem["rowindices"]), list(problem["colindices"]), problem["blocks"]
    else:
        rl = list(problem["diagonalindices"]) + list(problem["rowindices"])
        cl = list(problem["diagonalindices"]) + list(problem["colindices"])
        blocks = list(problem["diagonals"]) + list(problem["offdiagonals"])
    hull = lambda v: (int(np.min(v)), int(np.max(v))) if len(v) else None  # noqa: E731
    return [hull(v) for v in rl], [hull(v) for v in cl], [int(np.min(v)) if len(v) else 1 for v in rl], \
        [int(b.size) for b in blocks]


def partition_rule(nrows, keys, weights, nparts):
    """The row partition of both multi-GPU layers as include/bsm_rocm.h documents it (bsm_partition_rows), in numpy: the
    distinct keys, ascending, are cut into nparts contiguous ranges of about equal weight -- part p starts at the first
    key whose running weight in front of it reaches p / nparts of the total --; part p owns the rows from its first key
    to the next part's first key - 1 (the first part that has a key from row 1, the last one to nrows; a part without
    a key: an empty range just below the next part's first row; no block at all: part 0 owns everything).
    -> (part of every block, [(own_lo, own_hi)] 1-based inclusive)"""
    keys, weights = np.asarray(keys, dtype=np.int64), np.asarray(weights, dtype=np.int64)
    uk, kidx = np.unique(keys, return_inverse=True)
    nk = len(uk)
    w = np.zeros(nk, dtype=np.float64)
    np.add.at(w, kidx.reshape(-1), np.maximum(weights, 0).astype(np.float64))
    csum = np.concatenate([[0.0], np.cumsum(w)])
    cut = [0]
    for p in range(1, nparts):
        k = int(np.searchsorted(csum, csum[-1] * p / nparts, side="left"))
        cut.append(min(max(k, cut[-1]), nk))
    cut.append(nk)
    part_of_key = np.zeros(nk, dtype=np.int32)
    own = []
    for p in range(nparts):
        part_of_key[cut[p]:cut[p + 1]] = p
        if cut[p] == cut[p + 1]:
            lo = int(uk[cut[p]]) if cut[p] < nk else nrows + 1
            own.append([lo, lo - 1])
        else:
            own.append([int(uk[cut[p]]), int(uk[cut[p + 1]]) - 1 if cut[p + 1] < nk else nrows])
    have = [p for p in range(nparts) if cut[p] < cut[p + 1]]
    if have:
        own[have[0]][0], own[have[-1]][1] = 1, nrows
    else:
        own[0] = [1, nrows]
    return part_of_key[kidx.reshape(-1)] if nk else np.zeros(0, np.int32), [tuple(o) for o in own]


def partition_features(problem, parts):
    """which edges of the row partition into `parts` parts the operator reaches: "empty_part" (a part without a block),
    "halo_below" / "halo_above" (a part whose blocks write rows below / above the rows it owns -- through a row list, or
    through the column list of a symmetric off-diagonal block), "crossing_block" (VBCRS: a block that starts in a part's
    rows and ends behind them), "tall" / "wide" (more rows than columns / more columns than rows)"""
    rh, ch, keys, weights = block_lists(problem)
    part, own = partition_rule(problem["size"][0], keys, weights, parts)
    sym = problem["kind"] == "symmetric"
    out = set()
    for p in range(parts):
        mine = [b for b in range(len(keys)) if part[b] == p]
        if not mine:
            out.add("empty_part")
        lo, hi = own[p]
        for b in mine:
            for h in [rh[b]] + ([ch[b]] if sym else []):
                if h is None:
                    continue
                if h[0] < lo:
                    out.add("halo_below")
                if h[1] > hi:
                    out.add("halo_above")
                    if problem["kind"] == "vbcrs":
                        out.add("crossing_block")
    nr, nc = problem["size"]
    if nr != nc:
        out.add("tall" if nr > nc else "wide")
    return out


def seed_of(kind, dtype):
    """deterministic per (type, element type); BSM_FUZZ_OFFSET=k explores other streams"""
    import os
    off = int(os.environ.get("BSM_FUZZ_OFFSET", "0"))
    return (sum(map(ord, kind)) * 1000003 + sum(map(ord, np.dtype(dtype).str)) + 7919 * off) % (2 ** 32)
