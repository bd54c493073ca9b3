"""Entries of an operator: sub-matrices and the diagonal read out of the packed image (submatrices, submatrix, diag, and
A[I, J] through _getitem), and the COO / CSR export (rowcolvals, sparse from the mirror's blocks; rowcolvals_device,
sparse_device from the device image).  Imports matrices.py, which reaches _getitem here only when A[I, J] is called."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._marshal import _TORCH_OF, _empty, _host, _i64, _is_tensor, _p64, _ptrs, torch
from .matrices import (BlockSparseMatrix, SymmetricBlockMatrix, VariableBlockCompressedRowStorage, _operator, _unwrap, block,
                       colindices, colors, diagonal, diagonalcolors, diagonalindices, offdiagonal, offdiagonalcolors, rowindices,
                       size, transposeoffdiagonalcolors)

__all__ = ["rowcolvals", "sparse", "rowcolvals_device", "sparse_device", "submatrices", "submatrix", "diag"]


# ---- entries of the operator, read out of the packed image (bsm_submatrices / bsm_diag) ------------------------------
def _out_device(base):
    return torch.device("cuda", base.device if base.devices is None else base.devices[0])


def _out_space(base, device):
    """Where an extraction from `base` writes -> (dtype, device as _empty takes them, memspace, stream): numpy arrays in host
    memory, or (device=True) torch tensors on the handle's device, written on torch's current stream there."""
    if not device:
        return base.dtype, None, L.BSM_MEM_HOST, None
    if torch is None or base.device is None and base.devices is None:
        raise ValueError("device=True needs a handle with a device image")
    dev = _out_device(base)
    return _TORCH_OF[base.dtype], dev, L.BSM_MEM_DEVICE, torch.cuda.current_stream(dev).cuda_stream


def _addr(a):
    return a.data_ptr() if _is_tensor(a) else a.ctypes.data


def submatrices(A, rowsets, colsets=None, device=False):
    """[A[I_s, J_s] for s] in ONE pass over the packed image (bsm_submatrices).  rowsets / colsets: lists of 1-BASED
    index lists, like rowindices(A, i); colsets=None means the row sets again, so
    `submatrices(S, [diagonalindices(S, d) for d in eachdiagonalindex(S)])` gives the block-Jacobi blocks.  The row sets
    must be pairwise disjoint and free of repeats, and so must the column sets.  Overlapping blocks add, like sparse(A).
    Returns column-major numpy arrays; device=True: torch tensors on the handle's device, written there by the kernel
    on torch's current stream.  Synchronous.  transpose(A) / adjoint(A) are taken as such."""
    base, op = _operator(A)
    rs = [_i64(np.asarray(r).reshape(-1)) for r in rowsets]
    cs = rs if colsets is None else [_i64(np.asarray(c).reshape(-1)) for c in colsets]
    if len(rs) != len(cs):
        raise ValueError("one column set per row set")
    n = len(rs)
    ni, nj = _i64([len(r) for r in rs]), _i64([len(c) for c in cs])
    ld = np.maximum(ni, 1)
    dt, dev, memspace, st = _out_space(base, device)
    outs = [_empty(int(a), int(b), dt, dev) for a, b in zip(ni, nj)]
    outp = (C.c_void_p * max(n, 1))()
    for s, o in enumerate(outs):
        outp[s] = _addr(o) if ni[s] and nj[s] else None
    L.check(L.lib().bsm_submatrices(base._h.ptr, op, n, _ptrs(rs), _p64(ni), _ptrs(cs), _p64(nj), outp, _p64(ld), memspace, st))
    return outs


def submatrix(A, I, J, device=False):
    """A[I, J] for 1-BASED index lists without repeats (one set of submatrices)."""
    return submatrices(A, [I], [J], device)[0]


def diag(A, device=False):
    """LinearAlgebra.diag(A): the min(size) diagonal entries, read out of the packed image (bsm_diag); only the strips
    that cross the diagonal are loaded.  device=True: a torch tensor on the handle's device."""
    base, op = _operator(A)
    n = min(base.size)
    dt, dev, memspace, st = _out_space(base, device)
    d = _empty(n, None, dt, dev)
    L.check(L.lib().bsm_diag(base._h.ptr, _addr(d) if n else None, memspace, st))
    return d.conj() if op == L.BSM_OP_C and base.dtype.kind == "c" else d


def _getitem(A, key):
    """A[key] for every key but (:, :) -- see _LinearMap.__getitem__"""
    m, n = size(A)
    ri, ci = np.arange(m)[key[0]], np.arange(n)[key[1]]
    if np.ndim(ri) > 1 or np.ndim(ci) > 1:
        raise IndexError("an axis key must select a scalar or a 1-D set of indices")
    # repeated indices are extracted once and expanded here
    ru, rinv = np.unique(np.atleast_1d(ri), return_inverse=True)
    cu, cinv = np.unique(np.atleast_1d(ci), return_inverse=True)
    out = submatrix(A, ru + 1, cu + 1)[np.ix_(rinv.reshape(-1), cinv.reshape(-1))]
    if np.ndim(ci) == 0:
        out = out[:, 0]
    if np.ndim(ri) == 0:
        out = out[0]
    return out


# ---- conversion used by the reference's tests as their oracle (host utility, not the hot path) ----
def rowcolvals(A):
    """(rows, cols, vals), 1-based -- reference src/sparse.jl:17-123."""
    base, op = _unwrap(A)
    rows, cols, vals = [], [], []

    def push(b, ri, ci):  # _pushblocktoarrays!, src/sparse.jl:131-139 (row-major enumeration)
        R, Cc = np.meshgrid(np.asarray(ri), np.asarray(ci), indexing="ij")
        rows.append(R.ravel())
        cols.append(Cc.ravel())
        vals.append(_host(b).ravel())

    if isinstance(base, BlockSparseMatrix):
        for col in colors(A):
            for bid in col:
                push(block(A, bid), rowindices(A, bid), colindices(A, bid))
    elif isinstance(base, SymmetricBlockMatrix):
        for col in offdiagonalcolors(A):
            for bid in col:
                push(offdiagonal(A, bid), rowindices(A, bid), colindices(A, bid))
        for col in transposeoffdiagonalcolors(A):
            for bid in col:
                push(offdiagonal(A, bid).T, colindices(A, bid), rowindices(A, bid))
        for col in diagonalcolors(A):
            for bid in col:
                push(diagonal(A, bid), diagonalindices(A, bid), diagonalindices(A, bid))
    elif isinstance(base, VariableBlockCompressedRowStorage):
        if op != L.BSM_OP_N:
            raise NotImplementedError("rowcolvals of a wrapped VBCRS (the reference has none either)")
        for br in range(len(base.rowptr) - 1):
            for bi in range(base.rowptr[br], base.rowptr[br + 1]):
                b = _host(base.blocks[bi - 1])
                r0, c0 = base.rowindices[br], base.colindices[bi - 1]
                R, Cc = np.meshgrid(np.arange(r0, r0 + b.shape[0]), np.arange(c0, c0 + b.shape[1]),
                                    indexing="ij")
                rows.append(R.ravel(order="F"))
                cols.append(Cc.ravel(order="F"))
                vals.append(b.ravel(order="F"))
    else:
        raise TypeError("not a block matrix")
    if not rows:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0, base.dtype)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)


def rowcolvals_device(A, device=True):
    """bsm_rowcolvals: (rows, cols, vals), 1-based, written by a kernel from the packed DEVICE image
    (no block returns to the host).  device=True: torch CUDA tensors on the handle's device (multi-
    device handles: numpy arrays); False: numpy arrays.  Wrapped matrices: rows / cols swapped, values
    conjugated for the adjoint."""
    base, op = _unwrap(A)
    n = C.c_int64(0)
    L.check(L.lib().bsm_rowcolvals(base._h.ptr, None, None, None, C.byref(n), L.BSM_MEM_HOST, None))
    cnt = n.value
    on_dev = device and base.devices is None and torch is not None
    dev = torch.device("cuda", base.device) if on_dev else None
    kinds = (torch.int64, torch.int64, _TORCH_OF[base.dtype]) if on_dev else (np.int64, np.int64, base.dtype)
    r, c, v = (_empty(max(cnt, 1), None, t, dev) for t in kinds)
    L.check(L.lib().bsm_rowcolvals(base._h.ptr, _addr(r), _addr(c), _addr(v), C.byref(n), L.BSM_MEM_DEVICE if on_dev else L.BSM_MEM_HOST,
                                   torch.cuda.current_stream(dev).cuda_stream if on_dev else None))
    r, c, v = r[:cnt], c[:cnt], v[:cnt]
    if op != L.BSM_OP_N:
        r, c = c, r
        if op == L.BSM_OP_C:
            v = v.conj()
    return r, c, v


def sparse_device(A):
    """sparse(A) assembled ON the GPU: COO triples from the packed image (bsm_rowcolvals), duplicates
    summed and rows compressed by torch -> torch.sparse_csr_tensor on the handle's device
    (direct VBCRS -> CSR)."""
    r, c, v = rowcolvals_device(A, device=True)
    coo = torch.sparse_coo_tensor(torch.stack([r - 1, c - 1]), v, size=size(A)).coalesce()
    return coo.to_sparse_csr()


def sparse(A):
    """SparseArrays.sparse(A) -> scipy.sparse.csc_matrix (duplicates summed) -- src/sparse.jl:127-129."""
    import scipy.sparse as sp
    r, c, v = rowcolvals(A)
    return sp.coo_matrix((v, (r - 1, c - 1)), shape=size(A)).tocsc()
