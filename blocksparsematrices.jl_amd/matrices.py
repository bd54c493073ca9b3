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
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib as L

try:  # torch is plumbing only (device memory, streams)
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = [
    "SerialScheduler", "DynamicScheduler", "isserial", "AbstractBlockMatrix", "BlockSparseMatrix",
    "SymmetricBlockMatrix", "VariableBlockCompressedRowStorage", "TransposeMap", "AdjointMap",
    "transpose", "adjoint", "mul", "mul_parts", "MulPlan", "nnz", "size", "eltype", "scheduler", "block", "eachblockindex",
    "rowindices", "colindices", "colors", "transposecolors", "diagonal", "offdiagonal",
    "eachdiagonalindex", "eachoffdiagonalindex", "diagonalindices", "diagonalcolors",
    "offdiagonalcolors", "transposeoffdiagonalcolors", "rowcolvals", "sparse", "ColorInfo", "conflicts",
    "color", "coloringalgorithm", "Context", "partition_rows", "host_register", "host_unregister", "rowcolvals_device", "sparse_device",
    "update_blocks", "refresh", "submatrices", "submatrix", "diag", "invert_blocks", "BlockJacobi", "block_jacobi",
    "Gmres", "GmresInfo", "gmres", "krylov_orth", "krylov_orth_work", "Cg", "CgInfo", "cg", "cocg", "BiCgStab", "bicgstab", "GmresMulti",
]

_DT = {np.dtype(np.float32): L.BSM_F32, np.dtype(np.float64): L.BSM_F64,
       np.dtype(np.complex64): L.BSM_C64, np.dtype(np.complex128): L.BSM_C128}
# mixed precision (`storage=`): (vector / block type, stored type) -> dtype code
_MIXED = {(np.dtype(np.float64), np.dtype(np.float32)): L.BSM_F64_F32,
          (np.dtype(np.complex128), np.dtype(np.complex64)): L.BSM_C128_C64}


def _code(dt, storage, devices=None):
    """dtype code of a handle with blocks / vectors of type dt whose values are stored as `storage` (None: dt) ->
    (code, stored dtype).  Mixed precision stores Float64 blocks as Float32 (ComplexF64 as ComplexF32), rounded once
    at construction exactly like astype; products keep fp64 vectors and sums."""
    if storage is None:
        return _DT[dt], dt
    try:
        sdt = np.dtype(storage)
    except TypeError:
        raise TypeError(f"storage={storage!r} is not a dtype") from None
    if (dt, sdt) not in _MIXED:
        raise TypeError(f"storage={sdt} with {dt} blocks: mixed precision stores float64 blocks as float32 and "
                        f"complex128 blocks as complex64, nothing else")
    if devices is not None:
        raise ValueError("mixed-precision storage is single-device only (devices= is not available)")
    return _MIXED[(dt, sdt)], sdt


# ---- schedulers (OhMyThreads names; reference src/BlockSparseMatrices.jl:12-18) --------------
class SerialScheduler:
    def __repr__(self):
        return "SerialScheduler()"


class DynamicScheduler:
    def __repr__(self):
        return "DynamicScheduler()"


def isserial(s):
    return isinstance(s, SerialScheduler)


# ---- marshalling helpers -------------------------------------------------------------------------
def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptrs(arrs):
    out = (C.c_void_p * max(len(arrs), 1))()
    if len(arrs) and _is_dev(arrs):
        for i, a in enumerate(arrs):
            out[i] = a.data_ptr()
        return out
    for i, a in enumerate(arrs):
        out[i] = a.ctypes.data
    return out


_TORCH_DT = {}
if torch is not None:
    _TORCH_DT = {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64),
                 torch.complex64: np.dtype(np.complex64), torch.complex128: np.dtype(np.complex128)}
_TORCH_OF = {d: t for t, d in _TORCH_DT.items()}  # numpy dtype -> torch dtype


def _is_dev(blocks):
    """Blocks given as torch CUDA tensors: device-resident operator data (bsm_options.blocks_memspace
    = BSM_MEM_DEVICE), repacked by a kernel -- the Python stand-in for a Julia caller's ROCArrays."""
    return torch is not None and len(blocks) > 0 and isinstance(blocks[0], torch.Tensor) and blocks[0].is_cuda


def _dev_blocks(*blocklists):
    """Checks device-resident blocks (all CUDA tensors of one dtype and device, column-major) -> numpy dtype."""
    dt = dev = None
    for bl in blocklists:
        for b in bl:
            if not (isinstance(b, torch.Tensor) and b.is_cuda and b.dim() == 2):
                raise TypeError("device-resident blocks must all be 2-D torch CUDA tensors")
            if b.dtype not in _TORCH_DT or (dt is not None and _TORCH_DT[b.dtype] != dt):
                raise TypeError("device-resident blocks must share one supported element type")
            # (an empty block has no layout: torch gives a 0 x n tensor whatever strides its maker had)
            if b.numel() > 0 and (b.shape[0] > 1 and b.stride(0) != 1 or (b.shape[1] > 1 and b.stride(1) < b.shape[0])):
                raise TypeError("device-resident blocks must be column-major (e.g. torch.empty(n, m).t())")
            if dev is not None and b.device != dev:
                raise ValueError("device-resident blocks must live on one device")
            dt, dev = _TORCH_DT[b.dtype], b.device
    return dt


def _lds(blocks):
    """leading dimensions (elements) of column-major blocks"""
    if _is_dev(blocks):
        return _i64([max(b.stride(1) if b.shape[1] > 1 else b.shape[0], b.shape[0], 1) for b in blocks])
    return _i64([max(b.shape[0], 1) for b in blocks])


def _host(b):
    """numpy view of a block wherever it lives (accessors used by sparse() / rowcolvals())"""
    return b.cpu().numpy() if (torch is not None and isinstance(b, torch.Tensor)) else _dense(b)


def _dense(b):
    """A block as a numpy array.  The reference takes any AbstractMatrix as a block and counts it as prod(size)
    (`_nnz`, src/abstractblockmatrix.jl:65-71) -- sparse blocks included; here such a block (anything with
    `.toarray()`, e.g. a scipy.sparse matrix) is densified ONCE, at construction: the packed image holds dense
    panels anyway."""
    if hasattr(b, "toarray") and not isinstance(b, np.ndarray):
        b = b.toarray()
    return np.asarray(b)


def _blocks_dtype(*blocklists):
    dt = None
    for bl in blocklists:
        for b in bl:
            d = _dense(b).dtype if hasattr(b, "toarray") and not isinstance(b, np.ndarray) else np.asarray(b).dtype
            dt = d if dt is None else np.promote_types(dt, d)
    if dt is None:
        dt = np.dtype(np.float64)
    if dt not in _DT:
        dt = np.promote_types(dt, np.float32) if dt.kind in "iub" else dt
    if np.dtype(dt) == np.float16:  # (Julia would promote Float16 blocks with Float32 scalars the same way)
        dt = np.dtype(np.float32)
    if np.dtype(dt) not in _DT:
        raise TypeError(f"unsupported block element type {dt}")
    return np.dtype(dt)


def _fblocks(blocks, dt):
    out = []
    for b in blocks:
        a = _dense(b)
        if a.ndim != 2:
            raise ValueError("every block must be a 2-D array")
        out.append(np.asfortranarray(a, dtype=dt))
    return out


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
        devb = _is_dev(blocks)
        dt = _dev_blocks(blocks) if devb else _blocks_dtype(blocks)
        self.blocks = list(blocks) if devb else _fblocks(blocks, dt)
        self.rowindices = [_i64(r) for r in rowindices]
        self.colindices = [_i64(c) for c in colindices]
        nb = len(self.blocks)
        if len(self.rowindices) != nb or len(self.colindices) != nb:
            raise ValueError("blocks, rowindices and colindices must have equal lengths")
        for b, r, c in zip(self.blocks, self.rowindices, self.colindices):
            if b.shape != (len(r), len(c)):
                raise ValueError("block shape does not match its index lists")
        m = _i64([b.shape[0] for b in self.blocks])
        n = _i64([b.shape[1] for b in self.blocks])
        ld = _lds(self.blocks)
        dev = _default_device() if device is None else device
        code, sdt = _code(dt, storage, devices)
        o = _options(scheduler, dev, accumulate, own, transpose_image, devices, devb, coloringalgorithm)
        h = C.c_void_p()
        I = C.POINTER(C.c_int64)
        L.check(L.lib().bsm_blocksparse_create(
            code, int(size[0]), int(size[1]), nb, _ptrs(self.blocks), m.ctypes.data_as(I),
            n.ctypes.data_as(I), ld.ctypes.data_as(I), _ptrs(self.rowindices),
            _ptrs(self.colindices), C.byref(o), C.byref(h)))
        self._finish(h, dt, size, scheduler, dev, devices, sdt)
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
        devb = _is_dev(diagonals) or _is_dev(offdiagonals)
        dt = _dev_blocks(diagonals, offdiagonals) if devb else _blocks_dtype(diagonals, offdiagonals)
        self.diagonals = list(diagonals) if devb else _fblocks(diagonals, dt)
        self.diagonalindices = [_i64(d) for d in diagonalindices]
        self.offdiagonals = list(offdiagonals) if devb else _fblocks(offdiagonals, dt)
        self.rowindices = [_i64(r) for r in rowindices]
        self.colindices = [_i64(c) for c in colindices]
        nd, no = len(self.diagonals), len(self.offdiagonals)
        if len(self.diagonalindices) != nd or len(self.rowindices) != no or len(self.colindices) != no:
            raise ValueError("block and index list counts differ")
        for b, d in zip(self.diagonals, self.diagonalindices):
            if b.shape != (len(d), len(d)):
                raise ValueError("diagonal block shape does not match its index list")
        for b, r, c in zip(self.offdiagonals, self.rowindices, self.colindices):
            if b.shape != (len(r), len(c)):
                raise ValueError("off-diagonal block shape does not match its index lists")
        ds = _i64([b.shape[0] for b in self.diagonals])
        dld = _lds(self.diagonals)
        m = _i64([b.shape[0] for b in self.offdiagonals])
        n = _i64([b.shape[1] for b in self.offdiagonals])
        ld = _lds(self.offdiagonals)
        dev = _default_device() if device is None else device
        code, sdt = _code(dt, storage, devices)
        o = _options(scheduler, dev, accumulate, own, False, devices, devb)
        h = C.c_void_p()
        I = C.POINTER(C.c_int64)
        L.check(L.lib().bsm_symmetric_create(
            code, int(size[0]), int(size[1]), nd, _ptrs(self.diagonals), ds.ctypes.data_as(I),
            dld.ctypes.data_as(I), _ptrs(self.diagonalindices), no, _ptrs(self.offdiagonals),
            m.ctypes.data_as(I), n.ctypes.data_as(I), ld.ctypes.data_as(I),
            _ptrs(self.rowindices), _ptrs(self.colindices), C.byref(o), C.byref(h)))
        self._finish(h, dt, size, scheduler, dev, devices, sdt)
        self._src = lambda: list(self.diagonals) + list(self.offdiagonals)  # bsm_update_blocks order: diag..., off...
        self.offdiagonalcolors = _classes(self._bookkeeping(L.BSM_BK_COLORS))
        self.transposeoffdiagonalcolors = _classes(self._bookkeeping(L.BSM_BK_TRANSPOSECOLORS))
        self.diagonalcolors = _classes(self._bookkeeping(L.BSM_BK_DIAGONALCOLORS))


class VariableBlockCompressedRowStorage(AbstractBlockMatrix):
    """reference src/vbcrs.jl:36-199.  Fields: blocks (sorted), rowptr, colindices (per block),
    rowindices (per block row), size, scheduler -- all 1-based like the reference."""

    def __init__(self, matrices, rowindices=None, colindices=None, matrixsize=None, *,
                 scheduler=None, device=None, accumulate="auto", own=None, materialize=False,
                 transpose_image=False, devices=None, storage=None):
        """storage: np.float32 for float64 blocks / np.complex64 for complex128 ones stores the values in single
        precision under double-precision vectors (mixed precision).  A VBCRS made from a BlockSparseMatrix or a
        SymmetricBlockMatrix takes the source's storage type unless told otherwise."""
        I = C.POINTER(C.c_int64)
        if storage is None and isinstance(matrices, AbstractBlockMatrix) and matrices.storage_dtype != matrices.dtype:
            storage = matrices.storage_dtype
        h = C.c_void_p()
        dev = _default_device() if device is None else device
        if isinstance(matrices, SymmetricBlockMatrix) and not materialize:  # src/vbcrs.jl:189-264
            # Same bookkeeping as the reference's expansion [diagonals..., offdiagonals...,
            # transpose(offdiagonals)...] (:222-241), but the transposes are NOT materialised:
            # the device image is the symmetric one and each off-diagonal block is streamed once.
            s = matrices
            scheduler = s.scheduler if scheduler is None else scheduler
            dt = s.dtype
            mats = list(s.diagonals) + list(s.offdiagonals) + [o.T for o in s.offdiagonals]  # views
            ds = _i64([b.shape[0] for b in s.diagonals])
            dld = _lds(s.diagonals)
            d0 = _i64([int(d[0]) for d in s.diagonalindices])  # first(...), :231-239
            m = _i64([b.shape[0] for b in s.offdiagonals])
            n = _i64([b.shape[1] for b in s.offdiagonals])
            ld = _lds(s.offdiagonals)
            r0 = _i64([int(r[0]) for r in s.rowindices])
            c0 = _i64([int(c[0]) for c in s.colindices])
            code, sdt = _code(dt, storage, devices)
            o = _options(scheduler, dev, accumulate, own, False, devices,
                         _is_dev(s.diagonals) or _is_dev(s.offdiagonals))
            L.check(L.lib().bsm_vbcrs_create_from_symmetric(
                code, int(s.size[0]), int(s.size[1]), len(s.diagonals), _ptrs(s.diagonals),
                ds.ctypes.data_as(I), dld.ctypes.data_as(I), d0.ctypes.data_as(I), len(s.offdiagonals),
                _ptrs(s.offdiagonals), m.ctypes.data_as(I), n.ctypes.data_as(I), ld.ctypes.data_as(I),
                r0.ctypes.data_as(I), c0.ctypes.data_as(I), C.byref(o), C.byref(h)))
            matrixsize = s.size
            fb = mats
            src = lambda: list(s.diagonals) + list(s.offdiagonals)  # noqa: E731  the handle's block order
        else:
            materialized = False
            if isinstance(matrices, BlockSparseMatrix):  # src/vbcrs.jl:150-160
                # bsm_vbcrs_create_from_blocksparse: first(rowindices(b, i)) / first(colindices(b, i))
                # are taken inside the library (src/vbcrs.jl:201-215)
                b = matrices
                scheduler = b.scheduler if scheduler is None else scheduler
                if len(b.blocks) < 1:
                    raise IndexError("VariableBlockCompressedRowStorage needs at least one block")  # :81
                dt = b.dtype
                fb = b.blocks
                m = _i64([k.shape[0] for k in fb])
                n = _i64([k.shape[1] for k in fb])
                ld = _lds(fb)
                code, sdt = _code(dt, storage, devices)
                o = _options(scheduler, dev, accumulate, own, transpose_image, devices, _is_dev(fb))
                L.check(L.lib().bsm_vbcrs_create_from_blocksparse(
                    code, int(b.size[0]), int(b.size[1]), len(fb), _ptrs(fb), m.ctypes.data_as(I),
                    n.ctypes.data_as(I), ld.ctypes.data_as(I), _ptrs(b.rowindices), _ptrs(b.colindices),
                    C.byref(o), C.byref(h)))
                matrixsize = b.size
                mats = None
                src = lambda: list(b.blocks)  # noqa: E731  the source's own list: edits of b.blocks[i] are seen
            elif isinstance(matrices, SymmetricBlockMatrix):  # reference behaviour: materialise
                s = matrices
                scheduler = s.scheduler if scheduler is None else scheduler
                mats = list(s.diagonals) + list(s.offdiagonals) + [o.T for o in s.offdiagonals]
                materialized = True
                rowindices = ([int(d[0]) for d in s.diagonalindices] + [int(r[0]) for r in s.rowindices]
                              + [int(c[0]) for c in s.colindices])
                colindices = ([int(d[0]) for d in s.diagonalindices] + [int(c[0]) for c in s.colindices]
                              + [int(r[0]) for r in s.rowindices])
                matrixsize = s.size
            else:
                mats = matrices
            scheduler = SerialScheduler() if scheduler is None else scheduler
            if mats is not None:
                if len(mats) < 1:
                    raise IndexError("VariableBlockCompressedRowStorage needs at least one block")  # :81
                devb = _is_dev(mats)
                dt = _dev_blocks(mats) if devb else _blocks_dtype(mats)
                fb = list(mats) if devb else _fblocks(mats, dt)
                rs, cs = _i64(rowindices), _i64(colindices)
                if len(rs) != len(fb) or len(cs) != len(fb):
                    raise ValueError("matrices, rowindices and colindices must have equal lengths")
                m = _i64([b.shape[0] for b in fb])
                n = _i64([b.shape[1] for b in fb])
                ld = _lds(fb)
                code, sdt = _code(dt, storage, devices)
                o = _options(scheduler, dev, accumulate, own, transpose_image, devices, devb)
                L.check(L.lib().bsm_vbcrs_create(
                    code, int(matrixsize[0]), int(matrixsize[1]), len(fb), _ptrs(fb),
                    m.ctypes.data_as(I), n.ctypes.data_as(I), ld.ctypes.data_as(I), rs.ctypes.data_as(I),
                    cs.ctypes.data_as(I), C.byref(o), C.byref(h)))
                src = (lambda fb=fb: list(fb))  # the constructor's order (self.blocks is the sorted view of it)
                if materialized:
                    # the handle holds every off-diagonal block twice (as given and transposed): a new value for one
                    # must reach both, which no single entry of a block list expresses
                    def src():
                        raise NotImplementedError(
                            "update_blocks / refresh of a VBCRS that materialised a SymmetricBlockMatrix: build it with "
                            "materialize=False (the symmetric image, which refreshes from the source's lists)")
        self._finish(h, dt, matrixsize, scheduler, dev, devices, sdt)
        self._src = src
        self.perm = self._bookkeeping(L.BSM_BK_VBCRS_PERM).copy()
        self.rowptr = self._bookkeeping(L.BSM_BK_VBCRS_ROWPTR).copy()
        self.colindices = self._bookkeeping(L.BSM_BK_VBCRS_COLINDICES).copy()
        self.rowindices = self._bookkeeping(L.BSM_BK_VBCRS_ROWINDICES).copy()
        self.blocks = [fb[p - 1] for p in self.perm]


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


def _stream_ptr(stream, dev):
    if stream is not None:
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    return torch.cuda.current_stream(dev).cuda_stream if dev is not None else None


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
    if devb:
        if _dev_blocks(blks) != A.dtype:
            raise TypeError("device blocks must have the operator's element type")
        arrs = blks
    else:
        arrs = []
        for b in blks:
            a = _host(b)
            if a.ndim != 2 or not a.flags.f_contiguous or a.dtype != A.dtype:
                a = np.asfortranarray(a, dtype=A.dtype)
            arrs.append(a)
    ld = _lds(arrs)
    idv = _i64(ids)
    I = C.POINTER(C.c_int64)
    st = _stream_ptr(stream, blks[0].device) if devb and len(blks) else None
    L.check(L.lib().bsm_update_blocks(A._h.ptr, len(ids), idv.ctypes.data_as(I), _ptrs(arrs), ld.ctypes.data_as(I),
                                      L.BSM_MEM_DEVICE if devb else L.BSM_MEM_HOST, st))


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


# ---- mul! ------------------------------------------------------------------------------------------------
def _check_device(v, base, name):
    """A tensor on another GPU than the handle's would be dereferenced by kernels of the handle's
    device: a device memory fault that aborts the process.  Raise instead."""
    if base.devices is not None:  # multi-device handle: x / y may live on any device (peer copies)
        return
    if base.device is not None and v.device.index != base.device:
        raise ValueError(f"{name} lives on cuda:{v.device.index} but the matrix was created on cuda:{base.device}")


def _vec_info(v, dt, n, name, base=None):
    """-> (pointer, memspace, stream, keepalive)"""
    if torch is not None and isinstance(v, torch.Tensor) and v.is_cuda and base is not None:
        _check_device(v, base, name)
    if torch is not None and isinstance(v, torch.Tensor):
        if v.dim() != 1 or v.numel() != n:
            raise ValueError(f"DimensionMismatch: {name} has length {tuple(v.shape)}, expected {n}")
        tdt = _TORCH_OF[dt]
        if v.dtype != tdt or not v.is_contiguous():
            raise TypeError(f"{name} must be a contiguous {tdt} tensor")
        if v.is_cuda:
            return v.data_ptr(), L.BSM_MEM_DEVICE, torch.cuda.current_stream(v.device).cuda_stream, v
        a = v.numpy()
        return a.ctypes.data, L.BSM_MEM_HOST, None, a
    if not isinstance(v, np.ndarray):
        raise TypeError(f"{name} must be a numpy array or a torch tensor")
    if v.ndim != 1 or v.shape[0] != n:
        raise ValueError(f"DimensionMismatch: {name} has shape {v.shape}, expected ({n},)")
    if v.dtype != dt or not v.flags.c_contiguous:
        raise TypeError(f"{name} must be a contiguous {dt} array")
    return v.ctypes.data, L.BSM_MEM_HOST, None, v


def _mat_info(v, dt, n, name, base=None):
    """2-D column-major operand -> (pointer, ld, ncols, memspace, stream, keepalive)"""
    if torch is not None and isinstance(v, torch.Tensor) and v.is_cuda and base is not None:
        _check_device(v, base, name)
    if torch is not None and isinstance(v, torch.Tensor):
        tdt = _TORCH_OF[dt]
        if v.dim() != 2 or v.shape[0] != n:
            raise ValueError(f"DimensionMismatch: {name} has shape {tuple(v.shape)}, expected ({n}, k)")
        if v.dtype != tdt or v.stride(0) != 1 or (v.shape[1] > 1 and v.stride(1) < max(n, 1)):
            raise TypeError(f"{name} must be a column-major {tdt} tensor (e.g. torch.empty(k, n).t())")
        ld = v.stride(1) if v.shape[1] > 1 else max(n, 1)
        if v.is_cuda:
            return (v.data_ptr(), ld, v.shape[1], L.BSM_MEM_DEVICE,
                    torch.cuda.current_stream(v.device).cuda_stream, v)
        a = v.numpy()
        return a.ctypes.data, ld, v.shape[1], L.BSM_MEM_HOST, None, a
    if not isinstance(v, np.ndarray) or v.ndim != 2 or v.shape[0] != n:
        raise ValueError(f"DimensionMismatch: {name} must be a 2-D array with {n} rows")
    if v.dtype != dt or not v.flags.f_contiguous:
        raise TypeError(f"{name} must be a column-major (Fortran-order) {dt} array")
    return v.ctypes.data, max(n, 1), v.shape[1], L.BSM_MEM_HOST, None, v


# complex vectors under a real handle (bsm_mul_cvec / bsm_mul_multi_cvec): the supported (matrix, vector) pairs
_CVEC = {np.dtype(np.float32): np.dtype(np.complex64), np.dtype(np.float64): np.dtype(np.complex128)}
_CVEC_PAIRS = "supported pairs: (float64, complex128) and (float32, complex64)"


def _elt(v):
    """numpy dtype of a vector operand (None: neither a numpy array nor a torch tensor)"""
    if torch is not None and isinstance(v, torch.Tensor):
        return _TORCH_DT.get(v.dtype)
    return v.dtype if isinstance(v, np.ndarray) else None


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


def _mul_call(y, A, x, alpha, beta, multi=False, plan=False):
    """The one route of mul and MulPlan: resolves the vector type, checks the operands and builds the scalars ->
    (C function, its arguments but the stream, y's stream (None: host vectors), what must stay alive while they are
    used).  multi: x and y are column-major matrices (bsm_mul_multi, A streamed once per batch of columns instead of
    LinearMaps' column loop over _unsafe_mul!); plan: MulPlan, device-resident vectors only."""
    base, op = _unwrap(A)
    dt, cvec = _vec_type(base, x, y, alpha, beta)
    nr, nc = base.size
    ylen, xlen = (nr, nc) if op == L.BSM_OP_N else (nc, nr)
    if multi:
        xp, ldx, kx, xms, _, xkeep = _mat_info(x, dt, xlen, "X", base)
        yp, ldy, ky, yms, yst, ykeep = _mat_info(y, dt, ylen, "Y", base)
        if kx != ky:
            raise ValueError("DimensionMismatch: X and Y have different numbers of columns")
        if xms != yms:
            raise ValueError("X and Y must live in the same memory space")
        vecs = (kx, xp, ldx, yp, ldy)
    else:
        xp, xms, _, xkeep = _vec_info(x, dt, xlen, "x", base)
        yp, yms, yst, ykeep = _vec_info(y, dt, ylen, "y", base)
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
    base, _ = _unwrap(A)
    if not isinstance(base, AbstractBlockMatrix):
        raise TypeError("A must be a block matrix or its transpose/adjoint wrapper")
    multi = getattr(x, "ndim", 1) == 2 or getattr(y, "ndim", 1) == 2
    fn, args, st, _keep = _mul_call(y, A, x, alpha, beta, multi)
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
        self._fn, args, _, self._keep = _mul_call(y, A, x, alpha, beta, plan=True)
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
    if torch is not None and isinstance(x, torch.Tensor):
        if x.dim() == 2:  # A * X: column-major result
            y = torch.empty((x.shape[1], m), dtype=x.dtype, device=x.device).t()
            if x.stride(0) != 1:
                x = x.t().contiguous().t()
        else:
            y = torch.empty(m, dtype=x.dtype, device=x.device)
    else:
        dt = eltype(A)
        if np.iscomplexobj(x) and dt.kind != "c":  # complex vectors under a real matrix: a complex result
            dt = np.result_type(dt, np.asarray(x).dtype)
        x = np.asarray(x, dtype=dt)
        if x.ndim == 2:
            x = np.asfortranarray(x)
            y = np.empty((m, x.shape[1]), dtype=x.dtype, order="F")
        else:
            x = np.ascontiguousarray(x)
            y = np.empty(m, dtype=x.dtype)
    return mul(y, A, x)


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


# ---- entries of the operator, read out of the packed image (bsm_submatrices / bsm_diag) ------------------------------
def _out_device(base):
    return torch.device("cuda", base.device if base.devices is None else base.devices[0])


def submatrices(A, rowsets, colsets=None, device=False):
    """[A[I_s, J_s] for s] in ONE pass over the packed image (bsm_submatrices).  rowsets / colsets: lists of 1-BASED
    index lists, like rowindices(A, i); colsets=None means the row sets again, so
    `submatrices(S, [diagonalindices(S, d) for d in eachdiagonalindex(S)])` gives the block-Jacobi blocks.  The row sets
    must be pairwise disjoint and free of repeats, and so must the column sets.  Overlapping blocks add, like sparse(A).
    Returns column-major numpy arrays; device=True: torch tensors on the handle's device, written there by the kernel
    on torch's current stream.  Synchronous.  transpose(A) / adjoint(A) are taken as such."""
    base, op = _unwrap(A)
    if not isinstance(base, AbstractBlockMatrix):
        raise TypeError("A must be a block matrix or its transpose/adjoint wrapper")
    rs = [_i64(np.asarray(r).reshape(-1)) for r in rowsets]
    cs = rs if colsets is None else [_i64(np.asarray(c).reshape(-1)) for c in colsets]
    if len(rs) != len(cs):
        raise ValueError("one column set per row set")
    n, dt = len(rs), base.dtype
    ni, nj = _i64([len(r) for r in rs]), _i64([len(c) for c in cs])
    ld = np.maximum(ni, 1)
    outp = (C.c_void_p * max(n, 1))()
    st = None
    if device:
        if torch is None or base.device is None and base.devices is None:
            raise ValueError("device=True needs a handle with a device image")
        dev = _out_device(base)
        outs = [torch.empty((int(b), int(a)), dtype=_TORCH_OF[dt], device=dev).t() for a, b in zip(ni, nj)]
        for s, o in enumerate(outs):
            outp[s] = o.data_ptr() if o.numel() else None
        st = torch.cuda.current_stream(dev).cuda_stream
    else:
        outs = [np.empty((int(a), int(b)), dtype=dt, order="F") for a, b in zip(ni, nj)]
        for s, o in enumerate(outs):
            outp[s] = o.ctypes.data if o.size else None
    I = C.POINTER(C.c_int64)
    L.check(L.lib().bsm_submatrices(base._h.ptr, op, n, _ptrs(rs), ni.ctypes.data_as(I), _ptrs(cs), nj.ctypes.data_as(I),
                                    outp, ld.ctypes.data_as(I), L.BSM_MEM_DEVICE if device else L.BSM_MEM_HOST, st))
    return outs


def submatrix(A, I, J, device=False):
    """A[I, J] for 1-BASED index lists without repeats (one set of submatrices)."""
    return submatrices(A, [I], [J], device)[0]


def diag(A, device=False):
    """LinearAlgebra.diag(A): the min(size) diagonal entries, read out of the packed image (bsm_diag); only the strips
    that cross the diagonal are loaded.  device=True: a torch tensor on the handle's device."""
    base, op = _unwrap(A)
    if not isinstance(base, AbstractBlockMatrix):
        raise TypeError("A must be a block matrix or its transpose/adjoint wrapper")
    n, dt = min(base.size), base.dtype
    if device:
        if torch is None or base.device is None and base.devices is None:
            raise ValueError("device=True needs a handle with a device image")
        dev = _out_device(base)
        d = torch.empty(n, dtype=_TORCH_OF[dt], device=dev)
        L.check(L.lib().bsm_diag(base._h.ptr, d.data_ptr() if n else None, L.BSM_MEM_DEVICE,
                                 torch.cuda.current_stream(dev).cuda_stream))
    else:
        d = np.empty(n, dtype=dt)
        L.check(L.lib().bsm_diag(base._h.ptr, d.ctypes.data if n else None, L.BSM_MEM_HOST, None))
    return d.conj() if op == L.BSM_OP_C and dt.kind == "c" else d


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


# ---- block-Jacobi: the self-interaction blocks inverted where they are (bsm_invert_blocks) -----------------------------
def invert_blocks(blocks):
    """Inverts square column-major blocks IN PLACE (bsm_invert_blocks: Gauss-Jordan with partial row pivoting, one
    workgroup per block on the device, the same elimination serially for host blocks) -> info, one int64 per block:
    0, or the 1-based step whose pivot was zero or not finite (that block is then unspecified).  blocks: numpy arrays
    (Fortran order) or torch CUDA tensors (column-major, e.g. what submatrices(..., device=True) returns) of ONE
    element type and device, orders 0 .. 1024.  Device blocks go on torch's current stream; the call is synchronous."""
    blocks = list(blocks)
    nb = len(blocks)
    devb = _is_dev(blocks)
    if devb:
        dt = _dev_blocks(blocks)
    else:
        dt = None
        for b in blocks:
            if not (isinstance(b, np.ndarray) and b.ndim == 2 and b.dtype in _DT and b.flags.f_contiguous and b.flags.writeable):
                raise TypeError("host blocks must be writeable 2-D Fortran-order numpy arrays of a supported element type")
            if dt is not None and b.dtype != dt:
                raise TypeError("the blocks must share one element type")
            dt = b.dtype
    for b in blocks:
        if b.shape[0] != b.shape[1]:
            raise ValueError(f"a block of shape {tuple(b.shape)} is not square")
    info = np.zeros(max(nb, 1), dtype=np.int64)
    if nb == 0:
        return info[:0]
    n, ld = _i64([b.shape[0] for b in blocks]), _lds(blocks)
    ptrs = (C.c_void_p * nb)()
    for k, b in enumerate(blocks):
        if b.shape[0]:
            ptrs[k] = b.data_ptr() if devb else b.ctypes.data
    I = C.POINTER(C.c_int64)
    st = _stream_ptr(None, blocks[0].device) if devb else None
    L.check(L.lib().bsm_invert_blocks(_DT[dt], nb, ptrs, n.ctypes.data_as(I), ld.ctypes.data_as(I), info.ctypes.data_as(I),
                                      L.BSM_MEM_DEVICE if devb else L.BSM_MEM_HOST, st))
    return info


def _inverted_blocks(A, sets, stream=None):
    """[inv(A[I_s, I_s]) for s]: extracted where the image lives and inverted there (device tensors on the handle's first
    device, numpy arrays for an analysis-only handle)"""
    base, _ = _unwrap(A)
    on_dev = base.device is not None or base.devices is not None
    ctx = contextlib.nullcontext()
    if on_dev and stream is not None:
        st = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(stream)
        ctx = torch.cuda.stream(st)  # submatrices and invert_blocks both take torch's current stream
    with ctx:
        blocks = submatrices(A, sets, device=on_dev)
        info = invert_blocks(blocks)
    bad = np.nonzero(info)[0]
    if len(bad):
        raise np.linalg.LinAlgError(f"block_jacobi: A[I, I] of set {int(bad[0]) + 1} is singular to working precision (the pivot of "
                                    f"elimination step {int(info[bad[0]])} is zero or not finite)")
    return blocks


class BlockJacobi(BlockSparseMatrix):
    """M = sum_s E_s inv(A[I_s, I_s]) E_s^T -- the block-Jacobi (near-field) preconditioner of A as an ordinary
    BlockSparseMatrix handle: mul, M @ X, MulPlan, the wrappers, complex vectors under a real M and M[I, J] work as on
    any other.  Built by block_jacobi(A, sets).  Fields beside BlockSparseMatrix's: `sets` (1-based index arrays) and
    `source` (the A it was built from)."""

    def __init__(self, A, sets=None, *, storage=None, accumulate="auto", transpose_image=False):
        base, _ = _unwrap(A)
        if not isinstance(base, AbstractBlockMatrix):
            raise TypeError("A must be a block matrix or its transpose/adjoint wrapper")
        if sets is None:
            if not isinstance(base, SymmetricBlockMatrix):
                raise ValueError("sets=None means the diagonalindices of a SymmetricBlockMatrix; pass index sets for other types")
            sets = base.diagonalindices
        m, n = size(A)
        if m != n:
            raise ValueError(f"block_jacobi needs a square operator, size(A) = {(m, n)}")
        self.sets = [_i64(np.asarray(s).reshape(-1)) for s in sets]
        self.source = A
        blocks = _inverted_blocks(A, self.sets)
        dev = L.BSM_DEVICE_NONE if base.device is None and base.devices is None else _out_device(base).index
        super().__init__(blocks, self.sets, self.sets, (m, n), device=dev, storage=storage, accumulate=accumulate,
                         transpose_image=transpose_image)

    def refresh(self, A=None, stream=None):
        """Re-extracts the blocks of A (default: `source`, e.g. after update_blocks(A, ...)), inverts them and pushes them
        into this handle with update_blocks: no analysis, no reallocation of the image, the tensors of `blocks` stay.  A
        singular block raises LinAlgError and leaves M as it was; a `storage=` M raises what update_blocks raises."""
        _no_mixed_update(self)
        A = self.source if A is None else A
        if size(A) != self.size:
            raise ValueError(f"size(A) = {size(A)} but the preconditioner is {self.size}")
        update_blocks(self, _inverted_blocks(A, self.sets, stream), stream=stream)
        self.source = A


def block_jacobi(A, sets=None, *, storage=None, accumulate="auto", transpose_image=False):
    """The block-Jacobi preconditioner of A over `sets` (1-based index lists, pairwise disjoint and free of repeats;
    None: the diagonalindices of a SymmetricBlockMatrix) -> BlockJacobi.  submatrices(A, sets, device=True), invert_blocks
    and the BlockSparseMatrix constructor from device tensors: no matrix byte crosses PCIe.  An analysis-only A takes
    the same route on the host and gives an analysis-only M; a multi-device A gives a single-device M on its first
    device; transpose(A) / adjoint(A) are taken as such; a mixed-storage A gives its stored values widened, inverted in
    the vector type (storage= here is that of M).  Rows in no set are zero rows of M -- pass singleton sets for
    point-Jacobi rows.  A singular block raises numpy.linalg.LinAlgError naming the set and the elimination step."""
    return BlockJacobi(A, sets, storage=storage, accumulate=accumulate, transpose_image=transpose_image)


# ---- restarted GMRES on the device (bsm_gmres_*) and its building block (bsm_krylov_orth) ------------------------------
def krylov_orth_work(dtype, n, k):
    """Bytes of the `work` array one krylov_orth pass over n entries and k columns of `dtype` needs."""
    return int(L.lib().bsm_krylov_orth_work(_DT[np.dtype(dtype)], int(n), int(k)))


def krylov_orth(V, w, k, hsum, nrm, work=None, stream=None):
    """One classical Gram-Schmidt pass on the device (bsm_krylov_orth): h = V[:, :k]^H w, w -= V[:, :k] h, hsum[:k] += h,
    nrm[0] = ||w||.  V: column-major torch CUDA tensor (n x >= k, e.g. torch.empty(cols, ld).t()[:n]), w: n entries of the
    same type, hsum: >= k entries of it, nrm: one real of its precision, work: a uint8 tensor of krylov_orth_work bytes
    (None: allocated here).  Enqueued on `stream` (default: torch's current stream); nothing is synchronised."""
    if torch is None or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (V, w, hsum, nrm)):
        raise TypeError("krylov_orth takes torch CUDA tensors")
    dt = _TORCH_DT.get(w.dtype)
    if dt is None or V.dtype != w.dtype or hsum.dtype != w.dtype:
        raise TypeError("V, w and hsum must share one supported element type")
    if _TORCH_DT.get(nrm.dtype) != np.dtype(np.zeros(1, dt).real.dtype):
        raise TypeError(f"nrm must be one real of the precision of {dt}")
    if any(t.device != w.device for t in (V, hsum, nrm)):
        raise ValueError("V, w, hsum and nrm must live on one device")
    n, k = w.numel(), int(k)
    if w.dim() != 1 or not w.is_contiguous() or V.dim() != 2 or V.shape[0] != n:
        raise ValueError(f"DimensionMismatch: w must be a contiguous vector and V have its {n} rows")
    if not 0 <= k <= min(V.shape[1], L.BSM_GMRES_MAX_RESTART) or hsum.numel() < k or nrm.numel() < 1:
        raise ValueError(f"k = {k} outside 0 .. min(columns of V, {L.BSM_GMRES_MAX_RESTART}), or hsum shorter than k")
    if n > 1 and V.stride(0) != 1:
        raise TypeError("V must be column-major (e.g. torch.empty(cols, ld).t()[:n])")
    ldv = V.stride(1) if V.shape[1] > 1 else max(n, 1)
    need = krylov_orth_work(dt, n, k)
    if work is None:
        work = torch.empty(need + 16, dtype=torch.uint8, device=w.device)
    if work.device != w.device or work.numel() * work.element_size() < need:
        raise ValueError(f"work must hold {need} bytes on the device of w")
    L.check(L.lib().bsm_krylov_orth(_DT[dt], n, k, V.data_ptr(), ldv, w.data_ptr(), hsum.data_ptr(), nrm.data_ptr(),
                                    work.data_ptr(), _stream_ptr(stream, w.device)))
    return w


class GmresInfo:
    """What a solve reports (bsm_gmres_info): status (0 converged, 1 maxiter reached, 2 a non-finite residual),
    iterations, cycles, residual (absolute estimate), bnorm, a_products, m_products, workspace_bytes, workspace (device
    address) and history: the absolute estimate after every iteration, a numpy array."""

    def __init__(self, info, history):
        for name, _ in L.BsmGmresInfo._fields_:
            setattr(self, name, getattr(info, name))
        self.history = history

    @property
    def converged(self):
        return self.status == 0

    def __repr__(self):
        return (f"GmresInfo(status={self.status}, iterations={self.iterations}, cycles={self.cycles}, "
                f"residual={self.residual:.3e}, bnorm={self.bnorm:.3e})")


def _solver_operators(A, M, dtype):
    """the checks every solver object begins with -> (A's matrix, its op, M's matrix or None, its op, the vector type)"""
    base, op = _unwrap(A)
    if not isinstance(base, AbstractBlockMatrix):
        raise TypeError("A must be a block matrix or its transpose/adjoint wrapper")
    mbase, mop = (None, L.BSM_OP_N) if M is None else _unwrap(M)
    if M is not None and not isinstance(mbase, AbstractBlockMatrix):
        raise TypeError("M must be a block matrix or its transpose/adjoint wrapper")
    dtype = np.dtype(base.dtype if dtype is None else dtype)
    if dtype not in _DT:
        raise TypeError(f"dtype={dtype} is not a supported vector type")
    return base, op, mbase, mop, dtype


def _copy_guess(X, X0):
    """the initial guess X0 (torch tensor or numpy array, checked) into X, where the solver reads and overwrites it"""
    if X0 is X:
        return
    if torch is not None and isinstance(X, torch.Tensor):
        X.copy_(X0 if isinstance(X0, torch.Tensor) else torch.from_numpy(X0))
    else:
        X[...] = X0.cpu().numpy() if torch is not None and isinstance(X0, torch.Tensor) else X0


class Gmres:
    """Right-preconditioned restarted GMRES(restart) for A x = b, every step of it on the device (bsm_gmres_*: the
    solver of GmresMulti with one column behind its own info).
    A: a block matrix or transpose(A) / adjoint(A); M: a preconditioner of the same kind and order (e.g. block_jacobi(A,
    sets)), or None.  dtype: the type of b and x -- default A's vector type; a real A (and M) of the same precision
    takes complex vectors.  The workspace (restart + 3 vectors, restart + 4 with M) is allocated here, once; A and M are
    kept alive."""

    def __init__(self, A, M=None, restart=30, dtype=None):
        base, op, mbase, mop, self.dtype = _solver_operators(A, M, dtype)
        self.A, self.M, self.restart = A, M, int(restart)
        self.n = size(A)[0]
        self._base, self._mbase = base, mbase
        ptr = C.c_void_p()
        L.check(L.lib().bsm_gmres_create(base._h.ptr, op, None if mbase is None else mbase._h.ptr, mop, _DT[self.dtype],
                                         self.restart, C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr:
                L.lib().bsm_gmres_destroy(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def solve(self, b, x=None, x0=None, rtol=1e-8, atol=0.0, maxiter=None, stream=None):
        """-> (x, GmresInfo).  b: torch CUDA tensor (enqueued on `stream`, default torch's current stream) or numpy
        array (staged); x: where the solution goes (default: a new vector like b); x0: the initial guess (copied into x;
        None: zero).  Converged when the estimate is <= max(rtol * ||b||, atol); maxiter (default: the order of A)
        bounds the iterations.  Synchronous."""
        dev = torch is not None and isinstance(b, torch.Tensor) and b.is_cuda
        if x is None:
            x = torch.empty_like(b) if torch is not None and isinstance(b, torch.Tensor) else np.empty_like(b)
        bp, bms, _, bkeep = _vec_info(b, self.dtype, self.n, "b", self._base)
        xp, xms, _, xkeep = _vec_info(x, self.dtype, self.n, "x", self._base)
        if bms != xms:
            raise ValueError("b and x must live in the same memory space")
        if x0 is not None:
            if _elt(x0) != self.dtype or tuple(x0.shape) != (self.n,):
                raise TypeError(f"x0 must be a vector of {self.n} entries of {self.dtype}")
            _copy_guess(x, x0)
        maxiter = max(self.n, 1) if maxiter is None else int(maxiter)
        hist = np.zeros(max(maxiter, 1), dtype=np.float64)
        p = L.BsmGmresParams(C.sizeof(L.BsmGmresParams), 0 if x0 is None else 1, float(rtol), float(atol), maxiter, maxiter)
        info = L.BsmGmresInfo()
        st = _stream_ptr(stream, b.device) if dev else None
        if dev and stream is not None and x0 is not None and x0 is not x:
            torch.cuda.current_stream(b.device).synchronize()  # the copy of x0 went on torch's current stream
        L.check(L.lib().bsm_gmres_solve(self._ptr, bp, xp, C.byref(p), C.byref(info), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                        bms, st))
        del bkeep, xkeep
        return x, GmresInfo(info, hist[:min(info.iterations, maxiter)].copy())


def gmres(A, b, M=None, restart=30, **kw):
    """One-shot form: Gmres(A, M, restart, dtype of b).solve(b, **kw) -> (x, GmresInfo); a matrix B of k columns goes to
    GmresMulti(A, M, k, restart, dtype of B).solve(B, **kw) -> (X, CgInfo), its columns advancing in lockstep."""
    if getattr(b, "ndim", 1) == 2:
        return GmresMulti(A, M, nrhs=b.shape[1], restart=restart, dtype=_elt(b)).solve(b, **kw)
    return Gmres(A, M, restart=restart, dtype=_elt(b)).solve(b, **kw)


# ---- CG / COCG on several right-hand sides in lockstep, on the device (bsm_cg_*) -------------------------------------------
_CG_METHODS = {"cg": L.BSM_CG_METHOD_CG, "cocg": L.BSM_CG_METHOD_COCG}


class CgInfo:
    """What a solve reports (bsm_cg_info and the bsm_cg_column entries): status (the largest column status), iterations
    (the largest column count), columns_converged, a_products, m_products, workspace_bytes, workspace (device address);
    per column, as numpy arrays of k entries: column_status (0 converged, 1 maxiter reached, 2 a non-finite residual,
    3 breakdown), column_iterations, residual (absolute, by the recurrence), bnorm; history: (iterations, k), the
    residual norm of every column after every lockstep iteration (a finished column repeats its last value)."""

    def __init__(self, info, cols, history):
        for name, _ in L.BsmCgInfo._fields_:
            setattr(self, name, getattr(info, name))
        self.column_status = np.array([c.status for c in cols], dtype=np.int64)
        self.column_iterations = np.array([c.iterations for c in cols], dtype=np.int64)
        self.residual = np.array([c.residual for c in cols], dtype=np.float64)
        self.bnorm = np.array([c.bnorm for c in cols], dtype=np.float64)
        self.history = history

    @property
    def converged(self):
        return self.status == 0

    def __repr__(self):
        return (f"CgInfo(status={self.status}, iterations={self.iterations}, columns_converged={self.columns_converged} of "
                f"{len(self.column_status)}, column_iterations={self.column_iterations.tolist()})")


class _LockstepSolver:
    """What the lockstep solver objects (Cg, BiCgStab, GmresMulti) share: the checks and the create call, the destroy call, and solve().
    A subclass names its entry points in _abi (_abi + "_create" / "_solve" / "_destroy") and calls _setup()."""

    _abi = None

    def _setup(self, A, M, nrhs, dtype, extra=None):
        """the checks and the create call; extra(): called once A, M and dtype have passed, gives the arguments of create
        between nrhs_max and out"""
        base, op, mbase, mop, self.dtype = _solver_operators(A, M, dtype)
        extra = () if extra is None else extra()
        self.A, self.M, self.nrhs = A, M, int(nrhs)
        self.n = size(A)[0]
        self._base, self._mbase = base, mbase
        ptr = C.c_void_p()
        L.check(getattr(L.lib(), self._abi + "_create")(base._h.ptr, op, None if mbase is None else mbase._h.ptr, mop, _DT[self.dtype],
                                                        self.nrhs, *extra, C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr:
                getattr(L.lib(), self._abi + "_destroy")(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def _operand(self, v, name, vector):
        """-> (pointer, ld, columns, memspace, keepalive)"""
        if vector:
            ptr, ms, _, keep = _vec_info(v, self.dtype, self.n, name, self._base)
            return ptr, max(self.n, 1), 1, ms, keep
        ptr, ld, k, ms, _, keep = _mat_info(v, self.dtype, self.n, name, self._base)
        return ptr, ld, k, ms, keep

    history_capacity = 4096  # rows of CgInfo.history a solve keeps at the most (an attribute: set it on the solver to change it)

    def solve(self, B, X=None, X0=None, rtol=1e-8, atol=0.0, maxiter=None, stream=None, history=True):
        """-> (X, CgInfo).  B: a vector (n,) or a column-major matrix (n, k), k <= nrhs -- torch CUDA tensor (enqueued on
        `stream`, default torch's current stream) or numpy array (staged), taken as mul takes them; X: where the solution
        goes (default: new, like B); X0: the initial guess (copied into X; None: zero).  Column c is converged when its
        residual norm is <= max(rtol * ||b_c||, atol); maxiter (default: the order of A) bounds the lockstep iterations.
        A vector in gives a vector out.  info.history holds the first min(iterations, history_capacity = 4096) rows;
        history=False keeps none.  Synchronous."""
        is_t = torch is not None and isinstance(B, torch.Tensor)
        dev = is_t and B.is_cuda
        vector = getattr(B, "ndim", 1) == 1
        if X is None:
            if vector:
                X = torch.empty_like(B) if is_t else np.empty_like(B)
            elif is_t:
                X = torch.empty((B.shape[1], B.shape[0]), dtype=B.dtype, device=B.device).t()
            else:
                X = np.empty(B.shape, dtype=B.dtype, order="F")
        bp, ldb, k, bms, bkeep = self._operand(B, "B", vector)
        xp, ldx, kx, xms, xkeep = self._operand(X, "X", vector)
        if kx != k:
            raise ValueError("DimensionMismatch: B and X have different numbers of columns")
        if bms != xms:
            raise ValueError("B and X must live in the same memory space")
        if not 1 <= k <= self.nrhs:
            raise ValueError(f"B has {k} columns; this solver takes 1 .. {self.nrhs}")
        if X0 is not None:
            if _elt(X0) != self.dtype or tuple(X0.shape) != tuple(X.shape):
                raise TypeError(f"X0 must have the shape {tuple(X.shape)} and the type {self.dtype}")
            _copy_guess(X, X0)
        maxiter = max(self.n, 1) if maxiter is None else int(maxiter)
        cap = min(maxiter, self.history_capacity) if history else 0
        hist = np.empty((max(cap, 1), k), dtype=np.float64)
        p = L.BsmCgParams(C.sizeof(L.BsmCgParams), 0 if X0 is None else 1, float(rtol), float(atol), maxiter, cap)
        info = L.BsmCgInfo()
        cols = (L.BsmCgColumn * k)()
        st = _stream_ptr(stream, B.device) if dev else None
        if dev and stream is not None and X0 is not None and X0 is not X:
            torch.cuda.current_stream(B.device).synchronize()  # the copy of X0 went on torch's current stream
        L.check(getattr(L.lib(), self._abi + "_solve")(self._ptr, k, bp, ldb, xp, ldx, C.byref(p), C.byref(info), cols,
                                                       hist.ctypes.data_as(C.POINTER(C.c_double)), bms, st))
        del bkeep, xkeep
        return X, CgInfo(info, cols, hist[:min(info.iterations, cap)].copy())


class Cg(_LockstepSolver):
    """Preconditioned conjugate gradients for A X = B with up to `nrhs` right-hand sides advancing in lockstep on ONE
    multi-column product per iteration, every step on the device (bsm_cg_*).  method="cg": real symmetric / Hermitian
    positive definite A (and M); method="cocg": complex symmetric ones (the unconjugated form).  The CALLER asserts the
    symmetry.  A: a block matrix or transpose(A) / adjoint(A); M: a preconditioner of the same kind and order (e.g.
    block_jacobi(A, sets)), or None.  dtype: the type of B and X -- default A's vector type; a real A (and M) of the same
    precision takes complex vectors.  The workspace (4 n x nrhs matrices, 5 with M) is allocated here, once; A and M are
    kept alive."""

    _abi = "bsm_cg"

    def __init__(self, A, M=None, nrhs=1, dtype=None, method="cg"):
        def code():
            if method not in _CG_METHODS:
                raise ValueError(f"method={method!r}: 'cg' or 'cocg'")
            return (_CG_METHODS[method],)
        self._setup(A, M, nrhs, dtype, code)
        self.method = method


def _cg_oneshot(A, B, M, method, kw):
    k = 1 if getattr(B, "ndim", 1) == 1 else B.shape[1]
    return Cg(A, M, nrhs=k, dtype=_elt(B), method=method).solve(B, **kw)


def cg(A, B, M=None, **kw):
    """One-shot form: Cg(A, M, columns of B, dtype of B, "cg").solve(B, **kw) -> (X, info)."""
    return _cg_oneshot(A, B, M, "cg", kw)


def cocg(A, B, M=None, **kw):
    """One-shot form of the unconjugated method for complex symmetric A: Cg(..., method="cocg").solve(B, **kw)."""
    return _cg_oneshot(A, B, M, "cocg", kw)


# ---- BiCGSTAB on several right-hand sides in lockstep, on the device (bsm_bicgstab_*) ---------------------------------------
class BiCgStab(_LockstepSolver):
    """Right-preconditioned BiCGSTAB for A X = B with A NOT necessarily symmetric and up to `nrhs` right-hand sides
    advancing in lockstep on TWO multi-column products per iteration, every step on the device (bsm_bicgstab_*).  A: a
    block matrix or transpose(A) / adjoint(A); M: a preconditioner of the same kind and order (e.g. block_jacobi(A, sets)),
    or None.  dtype: the type of B and X -- default A's vector type; a real A (and M) of the same precision takes complex
    vectors.  The workspace (6 n x nrhs matrices, 7 with M) is allocated here, once; A and M are kept alive.  solve() is
    the one Cg has: the same arguments, (X, CgInfo) back; a column that converges after the first half of an iteration reports
    that half step's residual norm.  info.a_products = 2 * iterations (+ 1 with X0), m_products = 2 * iterations with M."""

    _abi = "bsm_bicgstab"

    def __init__(self, A, M=None, nrhs=1, dtype=None):
        self._setup(A, M, nrhs, dtype)


def bicgstab(A, B, M=None, **kw):
    """One-shot form: BiCgStab(A, M, columns of B, dtype of B).solve(B, **kw) -> (X, info)."""
    k = 1 if getattr(B, "ndim", 1) == 1 else B.shape[1]
    return BiCgStab(A, M, nrhs=k, dtype=_elt(B)).solve(B, **kw)


# ---- restarted GMRES on several right-hand sides in lockstep, on the device (bsm_gmres_multi_*) ----------------------------
class GmresMulti(_LockstepSolver):
    """Right-preconditioned restarted GMRES(restart) for A X = B with up to `nrhs` right-hand sides advancing in lockstep on
    ONE multi-column product per iteration, every step on the device (bsm_gmres_multi_*): per column the method of Gmres,
    all columns restarting together.  A: a block matrix or transpose(A) / adjoint(A); M: a preconditioner of the same kind
    and order (e.g. block_jacobi(A, sets)), or None.  dtype: the type of B and X -- default A's vector type; a real A (and
    M) of the same precision takes complex vectors.  The workspace (restart + 3 n x nrhs matrices, restart + 4 with M) is
    allocated here, once; A and M are kept alive.  solve() is the one Cg has: the same arguments, (X, CgInfo) back;
    info.history holds the residual ESTIMATES, info.cycles = ceil(iterations / restart); statuses 0, 1, 2 (never 3)."""

    _abi = "bsm_gmres_multi"

    def __init__(self, A, M=None, nrhs=1, restart=30, dtype=None):
        self.restart = int(restart)
        self._setup(A, M, nrhs, dtype, lambda: (self.restart,))

    def solve(self, B, **kw):
        X, info = super().solve(B, **kw)
        info.cycles = -(-int(info.iterations) // self.restart)
        return X, info


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
    dt = base.dtype
    if device and base.devices is None and torch is not None:
        tdt = {v: k for k, v in _TORCH_DT.items()}[dt]
        dev = torch.device("cuda", base.device)
        r = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
        c = torch.empty(max(cnt, 1), dtype=torch.int64, device=dev)
        v = torch.empty(max(cnt, 1), dtype=tdt, device=dev)
        L.check(L.lib().bsm_rowcolvals(base._h.ptr, r.data_ptr(), c.data_ptr(), v.data_ptr(), C.byref(n),
                                       L.BSM_MEM_DEVICE, torch.cuda.current_stream(dev).cuda_stream))
        r, c, v = r[:cnt], c[:cnt], v[:cnt]
        if op != L.BSM_OP_N:
            r, c = c, r
            if op == L.BSM_OP_C:
                v = v.conj()
        return r, c, v
    r = np.zeros(max(cnt, 1), dtype=np.int64)
    c = np.zeros(max(cnt, 1), dtype=np.int64)
    v = np.zeros(max(cnt, 1), dtype=dt)
    L.check(L.lib().bsm_rowcolvals(base._h.ptr, r.ctypes.data, c.ctypes.data, v.ctypes.data, C.byref(n),
                                   L.BSM_MEM_HOST, None))
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
