"""What the block-Jacobi suites (test_invert_blocks_cpu.py, test_gpu_invert_blocks.py, test_gpu_block_jacobi.py) share:
well-conditioned test blocks that need pivoting, the accuracy figure rho, a raw ctypes driver of bsm_invert_blocks and
operators of the three kinds whose self-interaction blocks A[I_s, I_s] are such blocks.  Test code only.

Blocks.  B = P (R + n I): R uniform in (-1, 1) (both parts for complex types), P a random row permutation, so the large
entries sit off the diagonal and every step of the elimination has to swap.  Condition numbers <= 2 for n = 1 .. 257.

Accuracy.  rho(X, B) = max|X B - I| / (n eps(T) max(|X| |B|)), evaluated in float64 / complex128.  A numpy emulation of
the elimination bsm_invert_blocks specifies and numpy.linalg.inv both stay <= 1.0 on these blocks over the sizes below,
3 draws, 4 types; the suites require rho <= RHO_MAX = 4 of the kernel and of the host path (the factor covers FMA
contraction, the reciprocal of a complex pivot and the update order on the device)."""
import ctypes as C

import numpy as np

from _submat import cut

SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 129, 255, 256, 257)
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
CODE = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.complex64): 2, np.dtype(np.complex128): 3}
RHO_MAX = 4.0
KINDS = ["blocksparse", "vbcrs", "symmetric"]


def uniform(rng, shape, dtype):
    r = rng.uniform(-1, 1, shape)
    if np.dtype(dtype).kind == "c":
        r = r + 1j * rng.uniform(-1, 1, shape)
    return r.astype(dtype)


def good_block(rng, n, dtype):
    """B = P (R + n I), column-major"""
    b = uniform(rng, (n, n), dtype) + n * np.eye(n, dtype=dtype)
    return np.asfortranarray(b[rng.permutation(n)])


def rho(X, B):
    n = B.shape[0]
    if n == 0:
        return 0.0
    wide = np.complex128 if np.dtype(B.dtype).kind == "c" else np.float64
    X64, B64 = np.asarray(X).astype(wide), np.asarray(B).astype(wide)
    res = np.max(np.abs(X64 @ B64 - np.eye(n)))
    scale = n * np.finfo(B.dtype).eps * np.max(np.abs(X64) @ np.abs(B64))
    return float(res / scale) if np.isfinite(res) else float("inf")


def padded(block, pad, guard=4):
    """the block inside a NaN-filled buffer with leading dimension n + pad and `guard` elements behind -> (buffer, view)"""
    n = block.shape[0]
    ld = max(n + pad, 1)
    buf = np.full(ld * n + guard, np.nan, dtype=block.dtype)
    view = buf[:ld * n].reshape(n, ld).T[:n, :]
    view[...] = block
    return buf, view


def outside(buf, n, ld):
    keep = np.ones(len(buf), dtype=bool)
    for j in range(n):
        keep[j * ld:j * ld + n] = False
    return buf[keep].tobytes()


def raw_invert(code, blocks, n, ld, info=True, memspace=0, stream=None, nblocks=None, null=()):
    """bsm_invert_blocks as C sees it -> (return code, info).  blocks: numpy buffers, device addresses or None;
    info=False passes NULL; null: names of the host arrays to pass as NULL ("blocks", "n", "ld")"""
    from bsm_amd import _lib as L
    nb = len(blocks) if nblocks is None else nblocks
    ptrs = (C.c_void_p * max(len(blocks), 1))()
    for k, b in enumerate(blocks):
        ptrs[k] = b.ctypes.data if isinstance(b, np.ndarray) else b
    nn, ll = np.ascontiguousarray(n, dtype=np.int64), np.ascontiguousarray(ld, dtype=np.int64)
    out = np.full(max(len(blocks), 1), -77, dtype=np.int64)
    P = C.POINTER(C.c_int64)
    rc = L.lib().bsm_invert_blocks(code, nb, None if "blocks" in null else ptrs, None if "n" in null else nn.ctypes.data_as(P),
                                   None if "ld" in null else ll.ctypes.data_as(P), out.ctypes.data_as(P) if info else None,
                                   memspace, stream)
    return rc, out[:len(blocks)]


# ---- operators whose self-interaction blocks are good blocks ------------------------------------------------------------
NOP = 400  # order of the operators: the sets of _submat.cut (1, 2, 7, 8, 9, 63, 64, 65, 129) and a rest of 52


def jacobi_problem(rng, kind, dtype, scale=1.0):
    """(problem, sets): an operator of order NOP and the scattered index sets of _submat.cut, built so that the SUM of
    the stored entries over every I_s x I_s is a good block: the block itself minus an extra block E that is stored
    beside it inside the 64-set (overlaps sum: main + E is the good block again), plus random coupling blocks between
    different sets, which a block-Jacobi preconditioner must ignore.  scale multiplies the good blocks (new values of
    the same layout for the refresh legs)."""
    sets = cut(rng, NOP)
    good = [good_block(rng, len(s), dtype) * dtype(scale) for s in sets]
    big = [k for k, s in enumerate(sets) if len(s) == 64][0]
    er, ec = np.arange(0, 5), np.arange(10, 17)  # positions inside the 64-set the extra block covers
    E = np.asfortranarray(uniform(rng, (len(er), len(ec)), dtype))
    pairs = [(a, b) for a in range(len(sets)) for b in range(len(sets)) if a != b]
    if kind == "vbcrs":
        # contiguous blocks only: the dense target (couplings everywhere outside the sets) cut into a 4 x 4 grid, the extra
        # block one more contiguous block laid over it
        D0 = uniform(rng, (NOP, NOP), dtype)
        for s, g in zip(sets, good):
            D0[np.ix_(s - 1, s - 1)] = g
        r0, c0 = 37, 211
        Ev = np.asfortranarray(uniform(rng, (23, 31), dtype))
        D0[r0:r0 + 23, c0:c0 + 31] -= Ev
        blocks, rs, cs = [], [], []
        for a in range(0, NOP, 100):
            for b in range(0, NOP, 100):
                blocks.append(np.asfortranarray(D0[a:a + 100, b:b + 100]))
                rs.append(a + 1)
                cs.append(b + 1)
        blocks.append(Ev)
        rs.append(r0 + 1)
        cs.append(c0 + 1)
        return dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rs, np.int64), colstart=np.array(cs, np.int64),
                    size=(NOP, NOP)), sets
    main = [g.copy(order="F") for g in good]
    main[big][np.ix_(er, ec)] -= E
    if kind == "blocksparse":
        blocks, ri, ci = list(main), list(sets), list(sets)
        blocks.append(E)
        ri.append(sets[big][er])
        ci.append(sets[big][ec])
        for k in rng.choice(len(pairs), size=12, replace=False):
            a, b = pairs[int(k)]
            ra, cb = sets[a][:max(1, len(sets[a]) // 2)], sets[b][len(sets[b]) // 3:]
            blocks.append(np.asfortranarray(uniform(rng, (len(ra), len(cb)), dtype)))
            ri.append(ra)
            ci.append(cb)
        return dict(kind="blocksparse", blocks=blocks, rowindices=ri, colindices=ci, size=(NOP, NOP)), sets
    # symmetric: an off-diagonal block counts at (r, c) and, transposed, at (c, r) -- the extra block inside the 64-set too
    main[big][np.ix_(ec, er)] -= E.T
    offs, ri, ci = [E], [sets[big][er]], [sets[big][ec]]
    for k in rng.choice(len(pairs), size=12, replace=False):
        a, b = pairs[int(k)]
        offs.append(np.asfortranarray(uniform(rng, (len(sets[a]), len(sets[b])), dtype)))
        ri.append(sets[a])
        ci.append(sets[b])
    return dict(kind="symmetric", diagonals=main, diagonalindices=list(sets), offdiagonals=offs, rowindices=ri, colindices=ci,
                size=(NOP, NOP)), sets


def set_blocks(D, sets):
    """[D[I_s, I_s] for s] of a dense array and 1-based index sets"""
    return [np.asfortranarray(D[np.ix_(np.asarray(s) - 1, np.asarray(s) - 1)]) for s in sets]


def dense_of(blocks, sets, n, dtype=None):
    """sum_s E_s blocks[s] E_s^T as a dense n x n array"""
    M = np.zeros((n, n), dtype=blocks[0].dtype if dtype is None else dtype)
    for b, s in zip(blocks, sets):
        M[np.ix_(np.asarray(s) - 1, np.asarray(s) - 1)] = b
    return M
