"""The five constructor routes the mixed-storage and complex-vector suites run over -- `blocksparse`, `vbcrs`, `symmetric`
and a VBCRS made from a BlockSparseMatrix / from a SymmetricBlockMatrix: a small problem per route (`ctor_problem`), its
handle (`ctor_build`) and the problem as the CPU oracle takes it (`ctor_oracle_problem`).  Test code only."""
import numpy as np

from _fuzz import cast_blocks

CTORS = ["blocksparse", "vbcrs", "symmetric", "vbcrs_from_blocksparse", "vbcrs_from_symmetric"]


def complexify(blocks, seed):
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(b + 1j * rng.standard_normal(b.shape)) for b in blocks]


def ctor_problem(bsm, ctor, dt, sizes):
    """A problem of the constructor's kind with blocks of type dt; sizes[ctor]: the keywords of its generator (config1 for
    `blocksparse`, config2 for `vbcrs` and `vbcrs_from_blocksparse`, config3 for the symmetric routes).  Complex dt: a
    seeded imaginary part is added to the generator's real blocks."""
    S = bsm.synthetic
    if ctor == "blocksparse":
        p = S.config1(**sizes[ctor])
    elif ctor == "vbcrs":
        p = S.config2(**sizes[ctor])
    elif ctor == "vbcrs_from_blocksparse":  # contiguous lists: the converter takes the first index of each
        v = S.config2(**sizes[ctor])
        p = dict(kind="blocksparse", blocks=v["blocks"], size=v["size"],
                 rowindices=[np.arange(r, r + b.shape[0], dtype=np.int64) for r, b in zip(v["rowstart"], v["blocks"])],
                 colindices=[np.arange(c, c + b.shape[1], dtype=np.int64) for c, b in zip(v["colstart"], v["blocks"])])
    else:
        p = S.config3(**sizes[ctor])
    if np.dtype(dt).kind == "c":
        for i, k in enumerate(("blocks",) if "blocks" in p else ("diagonals", "offdiagonals")):
            p[k] = complexify(p[k], 7 + i)
    return cast_blocks(p, dt)


def ctor_build(bsm, ctor, p, **kw):
    """Constructor `ctor` on problem p; the keywords go to the handle (a symmetric image has no transposed ordering:
    transpose_image is dropped there).  The source matrix of the two converting routes gets the handle's `device`."""
    if ctor in ("symmetric", "vbcrs_from_symmetric"):
        kw.pop("transpose_image", None)
    if not ctor.startswith("vbcrs_from_"):
        assert p["kind"] == ctor
        return bsm.synthetic.build(p, **kw)
    src = bsm.synthetic.build(p, **({"device": kw["device"]} if "device" in kw else {}))
    return bsm.matrices.VariableBlockCompressedRowStorage(src, **kw)


def ctor_oracle_problem(ctor, p):
    """the problem as the oracle takes it: a VBCRS from a BlockSparseMatrix / SymmetricBlockMatrix is the same operator"""
    if ctor == "vbcrs_from_symmetric":  # [diagonals..., offdiagonals..., transposes...] at the FIRST list entries
        d, o = p["diagonals"], p["offdiagonals"]
        first = lambda lists: [int(v[0]) for v in lists]  # noqa: E731
        rs = first(p["diagonalindices"]) + first(p["rowindices"]) + first(p["colindices"])
        cs = first(p["diagonalindices"]) + first(p["colindices"]) + first(p["rowindices"])
        return dict(kind="vbcrs", blocks=list(d) + list(o) + [np.asfortranarray(b.T) for b in o],
                    rowstart=np.array(rs, dtype=np.int64), colstart=np.array(cs, dtype=np.int64), size=p["size"])
    return p
