"""Host-side mirror of the reference's operator surface for the mul! hot path.

Same names, argument meaning and error behaviour as BlockSparseMatrices.jl:

    BlockSparseMatrix(blocks, rowindices, colindices, size; scheduler, coloringalgorithm)
        -- reference src/blockmatrix.jl:26-109
    SymmetricBlockMatrix(diagonals, diagonalindices, offdiagonals, rowindices, colindices,
                         size; scheduler)            -- src/symmetricblockmatrix.jl:33-126
    VariableBlockCompressedRowStorage(matrices, rowindices, colindices, size; scheduler)
    VariableBlockCompressedRowStorage(bsm | sbm)     -- src/vbcrs.jl:36-199
    mul(y, A, x[, alpha, beta])  == LinearAlgebra.mul!   (LinearMaps._unsafe_mul!)
    A @ x / A * x, transpose(A) / A.T, adjoint(A) / A.H  (LinearMaps wrappers, field .lmap)
    nnz, size, eltype, block, eachblockindex, rowindices, colindices, colors, ...

Julia conventions are kept on purpose so the parity tests read like the reference's tests:
index lists are 1-BASED, blocks are column-major 2-D arrays.  Every product runs in
libbsmrocm.so (HIP, gfx950); this module only marshals arguments.  x / y may be numpy
arrays (host memory: the library stages them over PCIe) or torch CUDA tensors (device
memory, enqueued on torch's current stream).

This module holds the operator types, the wrappers, colouring, the accessors, update_blocks / refresh and the
products.  The marshalling they share is in _marshal.py; entries of an operator and its COO / CSR export are in
entries.py, the block-Jacobi preconditioner and the Krylov solvers in solvers.py -- both import this module.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib as L
from ._marshal import (_BlockList, _TORCH_DT, _blocks_kind, _code, _describe, _dev_dtype, _elt, _host, _i64, _is_dev, _is_tensor,
                       _like, _p64, _ptrs, _stream_ptr, torch)

__all__ = [
    "SerialScheduler", "DynamicScheduler", "isserial", "AbstractBlockMatrix", "BlockSparseMatrix",
    "SymmetricBlockMatrix", "VariableBlockCompressedRowStorage", "TransposeMap", "AdjointMap",
    "transpose", "adjoint", "mul", "mul_parts", "MulPlan", "nnz", "size", "eltype", "scheduler", "block", "eachblockindex",
    "rowindices", "colindices", "colors", "transposecolors", "diagonal", "offdiagonal",
    "eachdiagonalindex", "eachoffdiagonalindex", "diagonalindices", "diagonalcolors",
    "offdiagonalcolors", "transposeoffdiagonalcolors", "ColorInfo", "conflicts",
    "color", "coloringalgorithm", "Context", "partition_rows", "host_register", "host_unregister", "update_blocks", "refresh",
]


# ---- schedulers (OhMyThreads names; reference src/BlockSparseMatrices.jl:12-18) --------------
class SerialScheduler:
    def __repr__(self):
        return "SerialScheduler()"


class DynamicScheduler:
    def __repr__(self):
        return "DynamicScheduler()"


def isserial(s):
    return isinstance(s, SerialScheduler)


class Context:
    """bsm_ctx_t: the GPUs of one node ONE handle is spread over (`devices=[0, 1, ...]` on any
    constructor).  The MI355X counterpart of the reference's `@tasks` fan-out over block rows /
    colour classes (src/vbcrs.jl:275-276, src/symmetricblockmatrix.jl:395-432).  The same ordinal may
    be listed several times (virtual devices)."""
    _cache = {}

    def __init__(self, devices):
        self.devices = tuple(int(d) for d in devices)
        ids = (C.c_int32 * len(self.devices))(*self.devices)
        h = C.c_void_p()
        L.check(L.lib().bsm_ctx_create(ids, len(self.devices), C.byref(h)))
        self.ptr = h

    @classmethod
    def get(cls, devices):
        """One context per device tuple for the life of the process (handles keep a pointer to it)."""
        key = tuple(int(d) for d in devices)
        if key not in cls._cache:
            cls._cache[key] = cls(key)
        return cls._cache[key]


def host_register(a):
    """bsm_host_register: page-locks a numpy vector used as x / y of host-memory products (DMA straight
    from / to it).  Keep `a` alive until host_unregister(a)."""
    L.check(L.lib().bsm_host_register(a.ctypes.data, a.nbytes))
    return a


def host_unregister(a):
    L.check(L.lib().bsm_host_unregister(a.ctypes.data))


def partition_rows(nrows, rowkeys, weights, nparts):
    """bsm_partition_rows: the row partition both multi-GPU layers use.  rowkeys[b] = smallest row
    index of block b (1-based), weights[b] = its stored entries.
    Returns (part_of_block, own) with own[p] = (lo, hi), 1-based inclusive (hi = lo - 1: empty)."""
    key, w = _i64(rowkeys), _i64(weights)
    nb = len(key)
    part = np.zeros(max(nb, 1), dtype=np.int32)
    lo, hi = np.zeros(nparts, dtype=np.int64), np.zeros(nparts, dtype=np.int64)
    I = C.POINTER(C.c_int64)
    L.check(L.lib().bsm_partition_rows(int(nrows), nb, key.ctypes.data_as(I), w.ctypes.data_as(I), int(nparts),
                                       part.ctypes.data_as(C.POINTER(C.c_int32)), lo.ctypes.data_as(I),
                                       hi.ctypes.data_as(I)))
    return part[:nb], [(int(a), int(b)) for a, b in zip(lo, hi)]


def _options(scheduler, device, accumulate, own=None, transpose_image=False, devices=None, dev_blocks=False,
             coloring=None):
    o = L.BsmOptions()
    L.lib().bsm_options_default(C.byref(o))
    o.scheduler = L.BSM_SCHED_SERIAL if isserial(scheduler) else L.BSM_SCHED_DYNAMIC
    o.device = device
    o.accumulate = {"auto": L.BSM_ACC_AUTO, "atomic": L.BSM_ACC_ATOMIC,
                    "colored": L.BSM_ACC_COLORED, "gather": L.BSM_ACC_GATHER,
                    "direct": L.BSM_ACC_DIRECT}[accumulate]
    if own is not None:
        o.own_lo, o.own_hi = int(own[0]), int(own[1])
    o.transpose_image = 2 if transpose_image == "auto" else (1 if transpose_image else 0)
    if devices is not None:
        if own is not None or transpose_image:
            raise ValueError("devices= does not combine with own= / transpose_image=")
        o.ctx = Context.get(devices).ptr
    o.blocks_memspace = L.BSM_MEM_DEVICE if dev_blocks else L.BSM_MEM_HOST
    o.coloring = _coloring_id(coloring)
    return o


def _default_device():
    """Current torch CUDA device when a GPU is visible, else analysis-only."""
    if torch is not None and torch.cuda.is_available():
        return torch.cuda.current_device()
    return L.BSM_DEVICE_NONE


def _scalar_buf(v, dt):
    return np.asarray([v], dtype=dt)


def _classes(flat):
    out, p = [], 1
    for _ in range(int(flat[0])):
        n = int(flat[p])
        out.append([int(v) for v in flat[p + 1:p + 1 + n]])
        p += 1 + n
    return out


class _Handle:
    """Owns a bsm_matrix_t; freed with the Python object (Julia side: a finalizer)."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                L.lib().bsm_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


# ---- LinearMaps-style base ---------------------------------------------------------------------------
class _LinearMap:
    """The slice of LinearMaps.LinearMap the reference relies on (`*`, mul!, adjoint, transpose)."""

    @property
    def shape(self):
        return size(self)

    def __matmul__(self, x):
        return _apply(self, x)

    def __mul__(self, x):
        return _apply(self, x)

    @property
    def T(self):
        return transpose(self)

    @property
    def H(self):
        return adjoint(self)

    def __getitem__(self, key):
        """A[:, :] -- LinearMaps materialises through products with unit vectors.
        Every other key reads the entries out of the packed image in one pass (submatrices): Python indexing, 0-BASED,
        each axis key taken as numpy takes it on that axis -- ints (negative ones too; an int drops its axis), slices
        with steps, integer arrays, boolean masks; a key numpy refuses raises what numpy raises.  Two index arrays
        select the sub-matrix A[np.ix_(I, J)] like the reference's A[I, J], not numpy's pointwise pairing."""
        if not (isinstance(key, tuple) and len(key) == 2):
            raise IndexError("a block matrix takes two indices: A[i, j]")
        if not all(isinstance(k, slice) and k == slice(None) for k in key):
            from .entries import _getitem  # entries.py imports this module, so not at the top of it
            return _getitem(self, key)
        m, n = size(self)
        dt = eltype(self)
        out = np.zeros((m, n), dtype=dt, order="F")
        step = 64  # unit vectors go through the multi-RHS entry (A streamed once per 8 of them)
        for j0 in range(0, n, step):
            k = min(step, n - j0)
            e = np.zeros((n, k), dtype=dt, order="F")
            e[np.arange(j0, j0 + k), np.arange(k)] = 1
            mul(out[:, j0:j0 + k], self, e)
        return out


class AbstractBlockMatrix(_LinearMap):
    """reference src/abstractblockmatrix.jl:13-62"""

    def _finish(self, handle, dt, sz, sched, device=None, devices=None, storage_dtype=None):
        self._h = _Handle(handle)
        self.dtype = dt
        # the type the device image stores the values in: dtype, or float32 / complex64 for a mixed-precision handle
        self.storage_dtype = dt if storage_dtype is None else storage_dtype
        self.size = (int(sz[0]), int(sz[1]))
        self.scheduler = sched
        self.devices = None if devices is None else tuple(int(d) for d in devices)
        self.device = None if (devices is not None or device == L.BSM_DEVICE_NONE) else int(device)

    def parts(self):
        """Per-device view of a multi-device handle: list of dicts (device, own, touched, ...)."""
        if self.devices is None:
            raise ValueError("not a multi-device handle")
        out = []
        for p in range(len(self.devices)):
            pi = L.BsmPartInfo()
            L.check(L.lib().bsm_part_info(self._h.ptr, p, C.byref(pi)))
            out.append(dict(device=pi.device, own=(pi.own_lo, pi.own_hi), touched=(pi.touched_lo, pi.touched_hi),
                            cols=(pi.col_lo, pi.col_hi), device_bytes=pi.device_bytes, nblocks=pi.nblocks))
        return out

    def stats(self):
        st = L.BsmStats()
        L.check(L.lib().bsm_stats(self._h.ptr, C.byref(st)))
        return {k: getattr(st, k) for k, _ in L.BsmStats._fields_ if k != "reserved"}

    def value_passes(self):
        """How many times products of this handle have streamed a value image since it was created (bsm_value_passes):
        a one-column product counts 1, a multi-column batch that streams the matrix once counts 1 whatever its width --
        so `A @ X` with K columns that adds K here ran column by column.  Counted when a product is enqueued (a captured
        one at capture).  Single-device handles."""
        n = C.c_int64(0)
        L.check(L.lib().bsm_value_passes(self._h.ptr, C.byref(n)))
        return n.value

    def _bookkeeping(self, which):
        n = C.c_int64(0)
        L.check(L.lib().bsm_get_bookkeeping(self._h.ptr, which, None, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        L.check(L.lib().bsm_get_bookkeeping(self._h.ptr, which,
                                            out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
        return out[:n.value]


class TransposeMap(_LinearMap):
    """LinearMaps.TransposeMap: lazy wrapper with field `.lmap`."""
    _op = L.BSM_OP_T

    def __init__(self, lmap):
        self.lmap = lmap


class AdjointMap(_LinearMap):
    """LinearMaps.AdjointMap: lazy wrapper with field `.lmap`."""
    _op = L.BSM_OP_C

    def __init__(self, lmap):
        self.lmap = lmap


def transpose(A):
    if isinstance(A, TransposeMap):
        return A.lmap
    if isinstance(A, AdjointMap):
        raise NotImplementedError("transpose(A') (= conj(A)) is not wrapped")
    return TransposeMap(A)


def adjoint(A):
    if isinstance(A, AdjointMap):
        return A.lmap
    if isinstance(A, TransposeMap):
        raise NotImplementedError("adjoint(transpose(A)) (= conj(A)) is not wrapped")
    return AdjointMap(A)


def _unwrap(A):
    if isinstance(A, (TransposeMap, AdjointMap)):
        return A.lmap, A._op
    return A, L.BSM_OP_N


def _operator(A, name="A"):
    """_unwrap for an argument that may be anything -> (the block matrix, op); TypeError if it is no block matrix"""
    base, op = _unwrap(A)
    if not isinstance(base, AbstractBlockMatrix):
        raise TypeError(f"{name} must be a block matrix or its transpose/adjoint wrapper")
    return base, op


# ---- colouring adapter (reference src/coloring.jl:15-61) ----------------------------------------------
# the reference's const (src/BlockSparseMatrices.jl:10); "DSATUR" selects plain DSATUR (GraphsColoring's names)
coloringalgorithm = "WorkstreamDSATUR"
_COLORING = {"WorkstreamDSATUR": L.BSM_COLOR_WORKSTREAM_DSATUR, "DSATUR": L.BSM_COLOR_DSATUR}


def _coloring_id(algorithm):
    name = coloringalgorithm if algorithm is None else algorithm
    if name not in _COLORING:
        raise ValueError(f"unknown coloring algorithm {name!r} (WorkstreamDSATUR, DSATUR)")
    return _COLORING[name]


class ColorInfo:
    """struct ColorInfo{R}: wraps the per-block conflict index lists (src/coloring.jl:15-17)."""

    def __init__(self, conflictindices):
        self.conflictindices = [_i64(c) for c in conflictindices]


class ConflictFunctor:
    def __init__(self, indices):
        self.indices = indices

    def __call__(self, i):
        return self.indices[i - 1]


def conflicts(blocks):
    """(eachindex(indices), ConflictFunctor(indices), Base.OneTo(maxconflict)) -- src/coloring.jl:45-61"""
    idx = blocks.conflictindices
    maxconflict = max(int(np.max(l)) for l in idx)
    return range(1, len(idx) + 1), ConflictFunctor(idx), range(1, maxconflict + 1)


def color(info, algorithm=None):
    """color(conflictgraph(info); algorithm).colors: classes of 1-based block ids that share no
    index (bsm_color; algorithm: "WorkstreamDSATUR" (default, like the reference) or "DSATUR")."""
    lists = info.conflictindices
    n = len(lists)
    lens = _i64([len(l) for l in lists])
    out = np.zeros(max(n, 1), dtype=np.int64)
    nc = C.c_int64(0)
    I = C.POINTER(C.c_int64)
    L.check(L.lib().bsm_color(n, _ptrs(lists), lens.ctypes.data_as(I), _coloring_id(algorithm),
                              out.ctypes.data_as(I), C.byref(nc)))
    return [[int(b) + 1 for b in np.nonzero(out[:n] == c)[0]] for c in range(nc.value)]


# ---- the three storage types ---------------------------------------------------------------------------
class BlockSparseMatrix(AbstractBlockMatrix):
    """reference src/blockmatrix.jl:26-109.  Fields: blocks, rowindices, colindices, size,
    colors, transposecolors, scheduler."""

    def __init__(self, blocks, rowindices, colindices, size, cols=None, *, scheduler=None,
                 coloringalgorithm=None, device=None, accumulate="auto", own=None,
                 transpose_image=False, devices=None, storage=None):
        if cols is not None:  # (blocks, rowindices, colindices, rows, cols) form, :81-89
            size = (size, cols)
        scheduler = SerialScheduler() if scheduler is None else scheduler
        bl = _BlockList(blocks)
        self.blocks = bl.blocks
        self.rowindices = [_i64(r) for r in rowindices]
        self.colindices = [_i64(c) for c in colindices]
        if len(self.rowindices) != len(bl) or len(self.colindices) != len(bl):
            raise ValueError("blocks, rowindices and colindices must have equal lengths")
        for b, r, c in zip(self.blocks, self.rowindices, self.colindices):
            if b.shape != (len(r), len(c)):
                raise ValueError("block shape does not match its index lists")
        dev = _default_device() if device is None else device
        code, sdt = _code(bl.dtype, storage, devices)
        o = _options(scheduler, dev, accumulate, own, transpose_image, devices, bl.dev, coloringalgorithm)
        h = C.c_void_p()
        L.check(L.lib().bsm_blocksparse_create(code, int(size[0]), int(size[1]), *bl.args(), _ptrs(self.rowindices),
                                               _ptrs(self.colindices), C.byref(o), C.byref(h)))
        self._finish(h, bl.dtype, size, scheduler, dev, devices, sdt)
        self._src = lambda: list(self.blocks)
        self.colors = _classes(self._bookkeeping(L.BSM_BK_COLORS))
        self.transposecolors = _classes(self._bookkeeping(L.BSM_BK_TRANSPOSECOLORS))


class SymmetricBlockMatrix(AbstractBlockMatrix):
    """reference src/symmetricblockmatrix.jl:33-126.  The tuple-size constructor defaults to
    DynamicScheduler() (:80)."""

    def __init__(self, diagonals, diagonalindices, offdiagonals, rowindices, colindices, size,
                 cols=None, *, scheduler=None, device=None, accumulate="auto", own=None, devices=None, storage=None):
        if cols is not None:  # rows, cols form defaults to SerialScheduler() (:102)
            size = (size, cols)
            scheduler = SerialScheduler() if scheduler is None else scheduler
        scheduler = DynamicScheduler() if scheduler is None else scheduler
        kind = _blocks_kind(diagonals, offdiagonals)
        dl = _BlockList(diagonals, kind)
        self.diagonals = dl.blocks
        self.diagonalindices = [_i64(d) for d in diagonalindices]
        ol = _BlockList(offdiagonals, kind)
        self.offdiagonals = ol.blocks
        self.rowindices = [_i64(r) for r in rowindices]
        self.colindices = [_i64(c) for c in colindices]
        if len(self.diagonalindices) != len(dl) or len(self.rowindices) != len(ol) or len(self.colindices) != len(ol):
            raise ValueError("block and index list counts differ")
        for b, d in zip(self.diagonals, self.diagonalindices):
            if b.shape != (len(d), len(d)):
                raise ValueError("diagonal block shape does not match its index list")
        for b, r, c in zip(self.offdiagonals, self.rowindices, self.colindices):
            if b.shape != (len(r), len(c)):
                raise ValueError("off-diagonal block shape does not match its index lists")
        dev = _default_device() if device is None else device
        code, sdt = _code(dl.dtype, storage, devices)
        o = _options(scheduler, dev, accumulate, own, False, devices, dl.dev)
        h = C.c_void_p()
        L.check(L.lib().bsm_symmetric_create(
            code, int(size[0]), int(size[1]), *dl.square_args(), _ptrs(self.diagonalindices), *ol.args(),
            _ptrs(self.rowindices), _ptrs(self.colindices), C.byref(o), C.byref(h)))
        self._finish(h, dl.dtype, size, scheduler, dev, devices, sdt)
        self._src = lambda: list(self.diagonals) + list(self.offdiagonals)  # bsm_update_blocks order: diag..., off...
        self.offdiagonalcolors = _classes(self._bookkeeping(L.BSM_BK_COLORS))
        self.transposeoffdiagonalcolors = _classes(self._bookkeeping(L.BSM_BK_TRANSPOSECOLORS))
        self.diagonalcolors = _classes(self._bookkeeping(L.BSM_BK_DIAGONALCOLORS))


# The four things a VariableBlockCompressedRowStorage is made from.  Each gives what the constructor's tail needs:
# (create call, its arguments between the size and the options -- they keep their arrays alive --, the (element type,
# device-resident) pair of the blocks, the block list `blocks` is the sorted view of, the `_src` callable of
# update_blocks / refresh, size, scheduler default, whether the call takes transpose_image).
_NO_BLOCK = "VariableBlockCompressedRowStorage needs at least one block"  # src/vbcrs.jl:81


def _first(lists):
    return [int(l[0]) for l in lists]


def _vbcrs_from_list(matrices, rowindices, colindices, matrixsize):
    if len(matrices) < 1:
        raise IndexError(_NO_BLOCK)
    bl = _BlockList(matrices)
    rs, cs = _i64(rowindices), _i64(colindices)
    if len(rs) != len(bl) or len(cs) != len(bl):
        raise ValueError("matrices, rowindices and colindices must have equal lengths")
    # _src: the constructor's order (blocks is the sorted view of it)
    return ("bsm_vbcrs_create", (*bl.args(), _p64(rs), _p64(cs)), (bl.dtype, bl.dev), bl.blocks, lambda: list(bl.blocks),
            matrixsize, SerialScheduler(), True)


def _vbcrs_from_blocksparse(b):  # src/vbcrs.jl:150-160
    """first(rowindices(b, i)) / first(colindices(b, i)) are taken inside the library (src/vbcrs.jl:201-215)"""
    if len(b.blocks) < 1:
        raise IndexError(_NO_BLOCK)
    bl = _BlockList(b.blocks, (b.dtype, _is_dev(b.blocks)))
    # _src: the source's own list, so that edits of b.blocks[i] are seen
    return ("bsm_vbcrs_create_from_blocksparse", (*bl.args(), _ptrs(b.rowindices), _ptrs(b.colindices)), (bl.dtype, bl.dev),
            bl.blocks, lambda: list(b.blocks), b.size, b.scheduler, True)


def _vbcrs_from_symmetric(s):  # src/vbcrs.jl:189-264
    """Same bookkeeping as the reference's expansion [diagonals..., offdiagonals..., transpose(offdiagonals)...] (:222-241),
    but the transposes are NOT materialised (views): the device image is the symmetric one and each off-diagonal block is
    streamed once."""
    kind = (s.dtype, _is_dev(s.diagonals) or _is_dev(s.offdiagonals))
    dl, ol = _BlockList(s.diagonals, kind), _BlockList(s.offdiagonals, kind)
    d0, r0, c0 = _i64(_first(s.diagonalindices)), _i64(_first(s.rowindices)), _i64(_first(s.colindices))  # first(...), :231-239
    # _src: the handle's block order
    return ("bsm_vbcrs_create_from_symmetric", (*dl.square_args(), _p64(d0), *ol.args(), _p64(r0), _p64(c0)), kind,
            dl.blocks + ol.blocks + [o.T for o in ol.blocks], lambda: list(s.diagonals) + list(s.offdiagonals), s.size,
            s.scheduler, False)


def _vbcrs_expanded(s):
    """the reference's behaviour: the expansion as a list of blocks"""
    d0, r0, c0 = _first(s.diagonalindices), _first(s.rowindices), _first(s.colindices)
    fn, args, kind, blocks, _, size, _, timg = _vbcrs_from_list(
        list(s.diagonals) + list(s.offdiagonals) + [o.T for o in s.offdiagonals], d0 + r0 + c0, d0 + c0 + r0, s.size)

    # the handle holds every off-diagonal block twice (as given and transposed): a new value for one must reach both,
    # which no single entry of a block list expresses
    def src():
        raise NotImplementedError(
            "update_blocks / refresh of a VBCRS that materialised a SymmetricBlockMatrix: build it with "
            "materialize=False (the symmetric image, which refreshes from the source's lists)")
    return fn, args, kind, blocks, src, size, s.scheduler, timg


class VariableBlockCompressedRowStorage(AbstractBlockMatrix):
    """reference src/vbcrs.jl:36-199.  Fields: blocks (sorted), rowptr, colindices (per block),
    rowindices (per block row), size, scheduler -- all 1-based like the reference."""

    def __init__(self, matrices, rowindices=None, colindices=None, matrixsize=None, *,
                 scheduler=None, device=None, accumulate="auto", own=None, materialize=False,
                 transpose_image=False, devices=None, storage=None):
        """storage: np.float32 for float64 blocks / np.complex64 for complex128 ones stores the values in single
        precision under double-precision vectors (mixed precision).  A VBCRS made from a BlockSparseMatrix or a
        SymmetricBlockMatrix takes the source's storage type unless told otherwise."""
        if storage is None and isinstance(matrices, AbstractBlockMatrix) and matrices.storage_dtype != matrices.dtype:
            storage = matrices.storage_dtype
        if isinstance(matrices, SymmetricBlockMatrix):
            source = _vbcrs_expanded(matrices) if materialize else _vbcrs_from_symmetric(matrices)
        elif isinstance(matrices, BlockSparseMatrix):
            source = _vbcrs_from_blocksparse(matrices)
        else:
            source = _vbcrs_from_list(matrices, rowindices, colindices, matrixsize)
        create, args, (dt, devb), blocks, src, matrixsize, default, timg = source
        scheduler = default if scheduler is None else scheduler
        dev = _default_device() if device is None else device
        code, sdt = _code(dt, storage, devices)
        o = _options(scheduler, dev, accumulate, own, transpose_image if timg else False, devices, devb)
        h = C.c_void_p()
        L.check(getattr(L.lib(), create)(code, int(matrixsize[0]), int(matrixsize[1]), *args, C.byref(o), C.byref(h)))
        self._finish(h, dt, matrixsize, scheduler, dev, devices, sdt)
        self._src = src
        self.perm = self._bookkeeping(L.BSM_BK_VBCRS_PERM).copy()
        self.rowptr = self._bookkeeping(L.BSM_BK_VBCRS_ROWPTR).copy()
        self.colindices = self._bookkeeping(L.BSM_BK_VBCRS_COLINDICES).copy()
        self.rowindices = self._bookkeeping(L.BSM_BK_VBCRS_ROWINDICES).copy()
        self.blocks = [blocks[p - 1] for p in self.perm]


# ---- new values for an existing operator (bsm_update_blocks) ----------------------------------------------
# The reference's types hold the caller's block matrices by reference (src/vbcrs.jl:98,114, src/blockmatrix.jl:26-34):
# an in-place edit of block(A, i) is what the next mul! reads.  The handle here holds a packed copy; these two calls
# bring it up to date without rebuilding it.  Block order = the constructor's: `blocks` of a BlockSparseMatrix or of
# a VBCRS made from a list (NOT its sorted A.blocks), diagonals + offdiagonals of a SymmetricBlockMatrix, and the
# source's lists for a VBCRS made from a BlockSparseMatrix / SymmetricBlockMatrix.
def _update_ids(ids, nb):
    if ids is None:
        return list(range(1, nb + 1))
    ids = [int(i) for i in ids]
    for i in ids:
        if not 1 <= i <= nb:
            raise IndexError(f"block id {i} out of range 1..{nb}")
    if len(set(ids)) != len(ids):
        raise ValueError("duplicate block id")
    return ids


def _no_mixed_update(A):
    if A.storage_dtype != A.dtype:
        raise NotImplementedError("update_blocks / refresh of a mixed-precision operator (storage="
                                  f"{A.storage_dtype} under {A.dtype}): build a new one from the new blocks")


def refresh(A, ids=None, stream=None):
    """Pushes the CURRENT contents of the mirror's block fields (A.blocks / A.diagonals / A.offdiagonals, edited in
    place by the caller) to the device image -- the reference's by-reference semantics, restored by one explicit call.
    ids: 1-based block ids in constructor order (None = all).  Device-resident blocks (torch CUDA tensors) are read by
    a kernel on `stream` (default: torch's current stream) without synchronising; host blocks are staged and the call
    returns when the image holds them."""
    A, _ = _unwrap(A)
    _no_mixed_update(A)
    src = A._src()
    ids = _update_ids(ids, len(src))
    blks = [src[i - 1] for i in ids]
    devb = _is_dev(blks)
    if devb and _dev_dtype(blks) != A.dtype:
        raise TypeError("device blocks must have the operator's element type")
    bl = _BlockList(blks, (A.dtype, devb), _host)
    st = _stream_ptr(stream, blks[0].device) if devb and len(blks) else None
    L.check(L.lib().bsm_update_blocks(A._h.ptr, len(ids), _p64(_i64(ids)), bl.ptrs, _p64(bl.ld), bl.memspace, st))


def update_blocks(A, blocks, ids=None, stream=None):
    """Replaces the values of blocks of A in place -- `copyto!(block(A, i), B)` for every new block, then one push to
    the device (refresh).  blocks: the new values in constructor order (for a SymmetricBlockMatrix diagonals +
    offdiagonals), numpy arrays or column-major torch CUDA tensors whatever A was built from; ids: their 1-based
    positions (None = all).  Shapes stay as created."""
    B, _ = _unwrap(A)
    _no_mixed_update(B)
    src = B._src()
    ids = _update_ids(ids, len(src))
    if len(blocks) != len(ids):
        raise ValueError("one block per id")
    for i, new in zip(ids, blocks):
        if tuple(new.shape) != tuple(src[i - 1].shape):
            raise ValueError(f"block {i}: shape {tuple(new.shape)} != {tuple(src[i - 1].shape)}")
    dev = [i for i in ids if torch is not None and isinstance(src[i - 1], torch.Tensor)]
    # the copies into device fields go on the stream the refill runs on (they must land before it reads them)
    ctx = contextlib.nullcontext()
    if dev and stream is not None:
        st = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(stream)
        st.wait_stream(torch.cuda.current_stream())  # the new values may come from the current stream's work
        ctx = torch.cuda.stream(st)
    with ctx:
        for i, new in zip(ids, blocks):
            dst = src[i - 1]
            if torch is not None and isinstance(dst, torch.Tensor):
                t = new if isinstance(new, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(new))
                dst.copy_(t.to(dst.device))
            else:
                dst[...] = new.cpu().numpy() if (torch is not None and isinstance(new, torch.Tensor)) else new
    refresh(B, ids, stream)


# complex vectors under a real handle (bsm_mul_cvec / bsm_mul_multi_cvec): the supported (matrix, vector) pairs
_CVEC = {np.dtype(np.float32): np.dtype(np.complex64), np.dtype(np.float64): np.dtype(np.complex128)}
_CVEC_PAIRS = "supported pairs: (float64, complex128) and (float32, complex64)"


def _vec_type(base, x, y, alpha, beta):
    """-> (vector dtype, complex vectors under a real handle).  Raises TypeError for the pairs nobody supports."""
    dt = base.dtype
    xt, yt = _elt(x), _elt(y)
    cx, cy = xt is not None and xt.kind == "c", yt is not None and yt.kind == "c"
    if dt.kind == "c" or not (cx or cy):
        if dt.kind != "c" and (np.iscomplexobj(alpha) or np.iscomplexobj(beta)):
            raise TypeError("complex alpha/beta with a real matrix need complex x and y (" + _CVEC_PAIRS + ")")
        return dt, False
    if base.storage_dtype != dt:
        raise TypeError(f"complex vectors under a mixed-storage matrix ({base.storage_dtype} under {dt}) are not "
                        "supported; " + _CVEC_PAIRS)
    if base.devices is not None:
        raise TypeError("complex vectors under a multi-device matrix are not supported; " + _CVEC_PAIRS)
    ct = _CVEC[dt]
    if xt != ct or yt != ct:
        raise TypeError(f"a {dt} matrix with x of {xt} and y of {yt}: " + _CVEC_PAIRS)
    return ct, True


def _scalars(alpha, beta, dt):
    """-> (alpha, beta as one-element arrays of dt, strong-zero flag): `beta is False` is Julia's strong zero"""
    strong = beta is False
    a = _scalar_buf(1 if alpha is True else alpha, dt)
    b = _scalar_buf(0 if strong else (1 if beta is True else beta), dt)
    return a, b, 1 if strong else 0


def _mul_call(y, base, op, x, alpha, beta, multi=False, plan=False):
    """The one route of mul and MulPlan for op(base): resolves the vector type, checks the operands and builds the
    scalars -> (C function, its arguments but the stream, y's stream (None: host vectors), what must stay alive while
    they are used).  multi: x and y are column-major matrices (bsm_mul_multi, A streamed once per batch of columns instead
    of LinearMaps' column loop over _unsafe_mul!); plan: MulPlan, device-resident vectors only."""
    dt, cvec = _vec_type(base, x, y, alpha, beta)
    nr, nc = base.size
    ylen, xlen = (nr, nc) if op == L.BSM_OP_N else (nc, nr)
    if multi:
        xp, ldx, kx, xms, _, xkeep = _describe(x, dt, xlen, "X", base, True)
        yp, ldy, ky, yms, yst, ykeep = _describe(y, dt, ylen, "Y", base, True)
        if kx != ky:
            raise ValueError("DimensionMismatch: X and Y have different numbers of columns")
        if xms != yms:
            raise ValueError("X and Y must live in the same memory space")
        vecs = (kx, xp, ldx, yp, ldy)
    else:
        xp, _, _, xms, _, xkeep = _describe(x, dt, xlen, "x", base)
        yp, _, _, yms, yst, ykeep = _describe(y, dt, ylen, "y", base)
        if plan and (xms != L.BSM_MEM_DEVICE or yms != L.BSM_MEM_DEVICE):
            raise ValueError("MulPlan needs device-resident x and y")
        if xms != yms:
            raise ValueError("x and y must live in the same memory space")
        vecs = (xp, yp)
    a, b, strong = _scalars(alpha, beta, dt)
    fn = getattr(L.lib(), "bsm_mul" + "_multi" * multi + "_cvec" * cvec)
    return fn, (base._h.ptr, op, *vecs, a.ctypes.data, b.ctypes.data, strong, xms), yst, (base, a, b, xkeep, ykeep)


def mul(y, A, x, alpha=True, beta=False):
    """LinearAlgebra.mul!(y, A, x, alpha, beta): y = alpha*A*x + beta*y, returns y.
    x / y may also be matrices (column-major): the multi right-hand-side product.  A real matrix takes complex x
    and y of its precision (float64 / complex128, float32 / complex64), with complex alpha / beta if wanted.

    `beta is False` (the 3-argument form, reference src/abstractblockmatrix.jl:27-34) is Julia's
    strong zero: y is overwritten, NaN/Inf in the incoming y do not propagate.  A numeric 0.0
    multiplies.  Dimension checks mirror LinearMaps' check_dim_mul (DimensionMismatch)."""
    base, op = _operator(A)
    multi = getattr(x, "ndim", 1) == 2 or getattr(y, "ndim", 1) == 2
    fn, args, st, _keep = _mul_call(y, base, op, x, alpha, beta, multi)
    L.check(fn(*args, st))
    return y


def mul_parts(y_parts, A, x_parts, alpha=True, beta=False):
    """bsm_mul_parts: mul!(y, A, x, alpha, beta) on a multi-device handle with x and y PARTITIONED over its
    devices.  x_parts[p] / y_parts[p]: torch CUDA tensors on the device of part p holding, for A (op N), the
    x entries of the part's column range (`A.parts()[p]["cols"]`) and the y entries of its row range
    (`["own"]`); for transpose(A) / adjoint(A) the other way round.  Enqueued on the current torch stream
    of every part's device; nothing is synchronised."""
    base, op = _unwrap(A)
    if base.devices is None:
        raise ValueError("mul_parts needs a multi-device handle (devices=[...])")
    dt = base.dtype
    parts = base.parts()
    if len(x_parts) != len(parts) or len(y_parts) != len(parts):
        raise ValueError("one x part and one y part per device of the handle")
    P = len(parts)
    xp, yp, st = (C.c_void_p * P)(), (C.c_void_p * P)(), (C.c_void_p * P)()
    for p, info in enumerate(parts):
        xr, yr = (info["cols"], info["own"]) if op == L.BSM_OP_N else (info["own"], info["cols"])
        for v, (lo, hi), name, arr in ((x_parts[p], xr, "x", xp), (y_parts[p], yr, "y", yp)):
            n = max(hi - lo + 1, 0)
            if v is None and n == 0:
                arr[p] = None
                continue
            if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 1 and v.is_contiguous()):
                raise TypeError(f"{name}_parts[{p}] must be a contiguous 1-D CUDA tensor")
            if v.numel() != n or _TORCH_DT.get(v.dtype) != dt:
                raise ValueError(f"DimensionMismatch: {name}_parts[{p}] has {v.numel()} entries of {v.dtype}, expected {n} of {dt}")
            if v.device.index != info["device"]:
                raise ValueError(f"{name}_parts[{p}] lives on cuda:{v.device.index}, part {p} on cuda:{info['device']}")
            arr[p] = v.data_ptr()
        st[p] = torch.cuda.current_stream(torch.device("cuda", info["device"])).cuda_stream
    a, b, strong = _scalars(alpha, beta, dt)
    L.check(L.lib().bsm_mul_parts(base._h.ptr, op, xp, yp, a.ctypes.data, b.ctypes.data, strong, st))
    return y_parts


class MulPlan:
    """Pre-marshalled mul!(y, A, x, alpha, beta) for device-resident x / y: `plan()` is one
    ctypes call into bsm_mul (no per-call Python marshalling), enqueued on the CURRENT torch
    stream -- what a Julia caller gets from `ccall` directly.  Graph-capturable."""

    def __init__(self, y, A, x, alpha=True, beta=False):
        self._fn, args, _, self._keep = _mul_call(y, *_unwrap(A), x, alpha, beta, plan=True)
        self._dev = y.device
        # (converted once, here: the call passes ready ctypes values)
        self._args = [args[0]] + [t(v) for t, v in zip(self._fn.argtypes[1:], args[1:])]

    def __call__(self):
        rc = self._fn(*self._args, C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream))
        if rc:
            L.check(rc)


class SegmentAdd:
    """Pre-marshalled `y[a_s : a_s + len_s] += src_s` over DISJOINT segments of one device vector, ONE launch on the
    current torch stream (bsm_vec_add_segments): the delivery step of distributed.RowPartitioned -- the own rows of the
    boundary blocks' sums + every received partial-y segment.  dsts: views of y, srcs: tensors of the same lengths."""

    def __init__(self, y, dsts, srcs):
        dt = {torch.float32: 0, torch.float64: 1, torch.complex64: 2, torch.complex128: 3}[y.dtype]
        es = y.element_size()
        n = len(dsts)
        for d, s_ in zip(dsts, srcs):
            if d.dtype != y.dtype or s_.dtype != y.dtype or d.shape != s_.shape or d.dim() != 1 or \
                    not d.is_contiguous() or not s_.is_contiguous() or d.device != y.device or s_.device != y.device:
                raise ValueError("segments must be contiguous 1-D tensors of y's type on y's device")
        # (an empty view has no address of its own)
        self._off = (C.c_int64 * n)(*[(d.data_ptr() - y.data_ptr()) // es if d.numel() else 0 for d in dsts])
        self._len = (C.c_int64 * n)(*[d.shape[0] for d in dsts])
        self._src = (C.c_void_p * n)(*[s_.data_ptr() if s_.numel() else None for s_ in srcs])
        if any(o < 0 or o + l_ > y.numel() for o, l_ in zip(self._off, self._len)):
            raise ValueError("a segment lies outside y")
        self._keep = (y, dsts, srcs)
        self._fn = L.lib().bsm_vec_add_segments
        self._args = [C.c_int(dt), C.c_void_p(y.data_ptr()), C.c_int32(n), self._off, self._src, self._len]
        self._dev = y.device

    def matches(self, y, dsts, srcs):
        ky, kd, ks = self._keep
        return ky.data_ptr() == y.data_ptr() and len(kd) == len(dsts) and \
            all(a.data_ptr() == b.data_ptr() and a.shape == b.shape for a, b in zip(kd, dsts)) and \
            all(a.data_ptr() == b.data_ptr() for a, b in zip(ks, srcs))

    def __call__(self):
        rc = self._fn(*self._args, C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream))
        if rc:
            L.check(rc)


def _apply(A, x):
    """A * x: allocates y like LinearMaps does (similar(x, ...), uninitialised) then mul!."""
    m, _ = size(A)
    if _is_tensor(x):
        if x.dim() == 2 and x.stride(0) != 1:  # A * X: column-major operand and result
            x = x.t().contiguous().t()
    else:
        dt = eltype(A)
        if np.iscomplexobj(x) and dt.kind != "c":  # complex vectors under a real matrix: a complex result
            dt = np.result_type(dt, np.asarray(x).dtype)
        x = np.asarray(x, dtype=dt)
        x = np.asfortranarray(x) if x.ndim == 2 else np.ascontiguousarray(x)
    return mul(_like(x, m, x.shape[1] if x.ndim == 2 else None), A, x)


# ---- accessors (reference names) ---------------------------------------------------------------------------
def size(A, dim=None):
    base, op = _unwrap(A)
    s = base.size if op == L.BSM_OP_N else (base.size[1], base.size[0])
    return s if dim is None else s[dim - 1]


def eltype(A):
    return _unwrap(A)[0].dtype


def scheduler(A):  # src/abstractblockmatrix.jl:50-62
    return _unwrap(A)[0].scheduler


def _wrapblock(b, op):
    if op == L.BSM_OP_T:
        return b.T
    if op == L.BSM_OP_C:
        return b.conj().T if not (torch is not None and isinstance(b, torch.Tensor)) else b.conj().t()
    return b


def eachblockindex(A):  # src/blockmatrix.jl:124-134
    return range(1, len(_unwrap(A)[0].blocks) + 1)


def block(A, i):  # src/blockmatrix.jl:150-160
    base, op = _unwrap(A)
    return _wrapblock(base.blocks[i - 1], op)


def rowindices(A, i):  # src/symmetricblockmatrix.jl:341-352
    base, op = _unwrap(A)
    return (base.rowindices if op == L.BSM_OP_N else base.colindices)[i - 1]


def colindices(A, i):  # src/symmetricblockmatrix.jl:354-365
    base, op = _unwrap(A)
    return (base.colindices if op == L.BSM_OP_N else base.rowindices)[i - 1]


def colors(A):  # src/blockmatrix.jl:177-206
    base, op = _unwrap(A)
    return base.colors if op == L.BSM_OP_N else base.transposecolors


def transposecolors(A):
    base, op = _unwrap(A)
    return base.transposecolors if op == L.BSM_OP_N else base.colors


def eachoffdiagonalindex(A):
    return range(1, len(_unwrap(A)[0].offdiagonals) + 1)


def eachdiagonalindex(A):
    return range(1, len(_unwrap(A)[0].diagonals) + 1)


def offdiagonal(A, i):  # src/symmetricblockmatrix.jl:199-237
    base, op = _unwrap(A)
    return _wrapblock(base.offdiagonals[i - 1], op)


def diagonal(A, i):
    base, op = _unwrap(A)
    return _wrapblock(base.diagonals[i - 1], op)


def diagonalindices(A, i):  # src/symmetricblockmatrix.jl:327-339
    return _unwrap(A)[0].diagonalindices[i - 1]


def diagonalcolors(A):
    return _unwrap(A)[0].diagonalcolors


def offdiagonalcolors(A):  # swaps for wrappers, src/symmetricblockmatrix.jl:307-325
    base, op = _unwrap(A)
    return base.offdiagonalcolors if op == L.BSM_OP_N else base.transposeoffdiagonalcolors


def transposeoffdiagonalcolors(A):
    base, op = _unwrap(A)
    return base.transposeoffdiagonalcolors if op == L.BSM_OP_N else base.offdiagonalcolors


def nnz(A):
    """SparseArrays.nnz -- src/blockmatrix.jl:208-223, src/symmetricblockmatrix.jl:367-384
    (off-diagonal blocks count twice), src/vbcrs.jl:290-296."""
    return int(_unwrap(A)[0].stats()["nnz"])
