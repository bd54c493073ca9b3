"""What every entry point of the Python layer does before it calls libbsmrocm.so, written once: the dtype tables, block
lists (`_BlockList`), vector / matrix operands (`_describe`), outputs (`_like`) and streams.  Private: matrices.py,
entries.py and solvers.py import from here, nothing here imports them."""
import ctypes as C

import numpy as np

from . import _lib as L

try:  # torch is plumbing only (device memory, streams)
    import torch
except Exception:  # pragma: no cover
    torch = None

_DT = {np.dtype(np.float32): L.BSM_F32, np.dtype(np.float64): L.BSM_F64,
       np.dtype(np.complex64): L.BSM_C64, np.dtype(np.complex128): L.BSM_C128}
# mixed precision (`storage=`): (vector / block type, stored type) -> dtype code
_MIXED = {(np.dtype(np.float64), np.dtype(np.float32)): L.BSM_F64_F32,
          (np.dtype(np.complex128), np.dtype(np.complex64)): L.BSM_C128_C64}
_TORCH_DT = {}
if torch is not None:
    _TORCH_DT = {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64),
                 torch.complex64: np.dtype(np.complex64), torch.complex128: np.dtype(np.complex128)}
_TORCH_OF = {d: t for t, d in _TORCH_DT.items()}  # numpy dtype -> torch dtype
_I64P = C.POINTER(C.c_int64)


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


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _p64(a):
    """an int64 array as the pointer a ctypes call takes (the pointer keeps the array alive)"""
    return a.ctypes.data_as(_I64P)


def _ptrs(arrs, dev=False):
    """the addresses of numpy arrays (dev: of torch CUDA tensors) as a void* array"""
    out = (C.c_void_p * max(len(arrs), 1))()
    if dev:
        for i, a in enumerate(arrs):
            out[i] = a.data_ptr()
    else:
        for i, a in enumerate(arrs):
            out[i] = a.ctypes.data
    return out


def _is_tensor(v):
    return torch is not None and isinstance(v, torch.Tensor)


# ---- block lists ---------------------------------------------------------------------------------------------------
def _is_dev(blocks):
    """Blocks given as torch CUDA tensors: device-resident operator data (bsm_options.blocks_memspace
    = BSM_MEM_DEVICE), repacked by a kernel -- the Python stand-in for a Julia caller's ROCArrays."""
    return torch is not None and len(blocks) > 0 and isinstance(blocks[0], torch.Tensor) and blocks[0].is_cuda


def _dev_dtype(*blocklists):
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


def _host(b):
    """numpy view of a block wherever it lives (accessors used by sparse() / rowcolvals())"""
    return b.cpu().numpy() if _is_tensor(b) else _dense(b)


def _dense(b):
    """A block as a numpy array.  The reference takes any AbstractMatrix as a block and counts it as prod(size)
    (`_nnz`, src/abstractblockmatrix.jl:65-71) -- sparse blocks included; here such a block (anything with
    `.toarray()`, e.g. a scipy.sparse matrix) is densified ONCE, at construction: the packed image holds dense
    panels anyway."""
    if hasattr(b, "toarray") and not isinstance(b, np.ndarray):
        b = b.toarray()
    return np.asarray(b)


def _host_dtype(*blocklists):
    dt = None
    for bl in blocklists:
        for b in bl:
            d = _dense(b).dtype
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


def _blocks_kind(*blocklists):
    """The block lists of ONE operator, checked -> (their common element type, device-resident)."""
    dev = any(_is_dev(bl) for bl in blocklists)
    return (_dev_dtype if dev else _host_dtype)(*blocklists), dev


class _BlockList:
    """One list of column-major blocks as a ctypes call takes it.  kind: (element type, device-resident) when the caller
    has settled it (_blocks_kind over several lists, or the operator's own type), else found and checked here.  Device
    blocks are taken as they are; host blocks become Fortran-order numpy arrays of the element type (`dense` makes a
    numpy array of one first), without a copy where they are that already.  Fields: blocks (kept alive with this
    object), dtype, dev, memspace, the int64 arrays m, n (shapes) and ld (leading dimensions, elements), ptrs."""

    def __init__(self, blocks, kind=None, dense=_dense):
        self.dtype, self.dev = _blocks_kind(blocks) if kind is None else kind
        if self.dev:
            self.blocks = list(blocks)
        else:
            self.blocks = []
            for b in blocks:
                a = dense(b)
                if a.ndim != 2:
                    raise ValueError("every block must be a 2-D array")
                self.blocks.append(np.asfortranarray(a, dtype=self.dtype))
        self.memspace = L.BSM_MEM_DEVICE if self.dev else L.BSM_MEM_HOST
        # (generators, not a list of the shapes: refresh may run under stream capture, and no more objects than before
        # should be alive at once there -- docs/experiments_r30.md has the one failure that led to this, and what is
        # only supposed about it)
        nb = len(self.blocks)
        self.m = np.fromiter((b.shape[0] for b in self.blocks), np.int64, nb)
        self.n = np.fromiter((b.shape[1] for b in self.blocks), np.int64, nb)
        self.ld = np.maximum(self.m, 1)
        if self.dev:  # a view's columns may lie further apart than its rows
            self.ld = np.maximum(self.ld, _i64([b.stride(1) if b.shape[1] > 1 else 0 for b in self.blocks]))
        self.ptrs = _ptrs(self.blocks, self.dev)

    def __len__(self):
        return len(self.blocks)

    def args(self):
        """count, blocks, m, n, ld: the arguments of a create call for this list"""
        return len(self.blocks), self.ptrs, _p64(self.m), _p64(self.n), _p64(self.ld)

    def square_args(self):
        """count, blocks, order, ld: the same for a list of square blocks"""
        return len(self.blocks), self.ptrs, _p64(self.m), _p64(self.ld)


# ---- operands, outputs, streams --------------------------------------------------------------------------------------
def _check_device(v, base, name):
    """A tensor on another GPU than the handle's would be dereferenced by kernels of the handle's
    device: a device memory fault that aborts the process.  Raise instead."""
    if base.devices is not None:  # multi-device handle: x / y may live on any device (peer copies)
        return
    if base.device is not None and v.device.index != base.device:
        raise ValueError(f"{name} lives on cuda:{v.device.index} but the matrix was created on cuda:{base.device}")


def _describe(v, dt, n, name, base=None, matrix=False):
    """The operand `name` of a product or a solve, checked: a contiguous vector of n entries of dt, or with matrix a
    column-major matrix of n rows -> (pointer, ld, columns, memspace, stream, keepalive); stream: torch's current one on
    the device of a CUDA tensor, None for host memory.  base: the operator whose device a CUDA tensor must live on."""
    if torch is not None and isinstance(v, torch.Tensor):  # (spelled out: every eager product comes through here twice)
        if v.is_cuda and base is not None:
            _check_device(v, base, name)
        tdt = _TORCH_OF[dt]
        if matrix:
            if v.dim() != 2 or v.shape[0] != n:
                raise ValueError(f"DimensionMismatch: {name} has shape {tuple(v.shape)}, expected ({n}, k)")
            if v.dtype != tdt or v.stride(0) != 1 or (v.shape[1] > 1 and v.stride(1) < (n or 1)):
                raise TypeError(f"{name} must be a column-major {tdt} tensor (e.g. torch.empty(k, n).t())")
            ld, k = v.stride(1) if v.shape[1] > 1 else n or 1, v.shape[1]
        else:
            if v.dim() != 1 or v.numel() != n:
                raise ValueError(f"DimensionMismatch: {name} has length {tuple(v.shape)}, expected {n}")
            if v.dtype != tdt or not v.is_contiguous():
                raise TypeError(f"{name} must be a contiguous {tdt} tensor")
            ld, k = n or 1, 1
        if v.is_cuda:
            return v.data_ptr(), ld, k, L.BSM_MEM_DEVICE, torch.cuda.current_stream(v.device).cuda_stream, v
        v = v.numpy()
    elif matrix:
        if not isinstance(v, np.ndarray) or v.ndim != 2 or v.shape[0] != n:
            raise ValueError(f"DimensionMismatch: {name} must be a 2-D array with {n} rows")
        if v.dtype != dt or not v.flags.f_contiguous:
            raise TypeError(f"{name} must be a column-major (Fortran-order) {dt} array")
        ld, k = n or 1, v.shape[1]
    else:
        if not isinstance(v, np.ndarray):
            raise TypeError(f"{name} must be a numpy array or a torch tensor")
        if v.ndim != 1 or v.shape[0] != n:
            raise ValueError(f"DimensionMismatch: {name} has shape {v.shape}, expected ({n},)")
        if v.dtype != dt or not v.flags.c_contiguous:
            raise TypeError(f"{name} must be a contiguous {dt} array")
        ld, k = n or 1, 1
    return v.ctypes.data, ld, k, L.BSM_MEM_HOST, None, v


def _elt(v):
    """numpy dtype of a vector operand (None: neither a numpy array nor a torch tensor)"""
    if _is_tensor(v):
        return _TORCH_DT.get(v.dtype)
    return v.dtype if isinstance(v, np.ndarray) else None


def _empty(rows, cols, dtype, device=None):
    """An uninitialised output: a vector of `rows` entries, or (cols not None) a column-major rows x cols matrix.  A numpy
    array of the numpy `dtype`; with `device` a torch tensor of the torch `dtype` there, a matrix as the .t() of a
    contiguous one."""
    if device is not None:
        if cols is None:
            return torch.empty(rows, dtype=dtype, device=device)
        return torch.empty((cols, rows), dtype=dtype, device=device).t()
    return np.empty(rows, dtype=dtype) if cols is None else np.empty((rows, cols), dtype=dtype, order="F")


def _like(v, rows, cols=None):
    """an output like the operand v -- its library, element type and device -- with `rows` rows (see _empty)"""
    return _empty(rows, cols, v.dtype, v.device if _is_tensor(v) else None)


def _stream_ptr(stream, dev):
    if stream is not None:
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    return torch.cuda.current_stream(dev).cuda_stream if dev is not None else None
