"""The block-Jacobi preconditioner (invert_blocks, eigh_blocks, spectral_blocks, BlockJacobi, block_jacobi) and the Krylov solvers that run every step
on the device: the Gram-Schmidt pass krylov_orth, Gmres, and the lockstep solvers Cg, BiCgStab, Minres, GmresMulti, Lsqr with
their one-shot forms.  The solver objects share _Solver: the create and destroy calls and the prelude of solve()."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib as L
from ._marshal import _BlockList, _DT, _TORCH_DT, _TORCH_OF, _blocks_kind, _describe, _elt, _i64, _is_dev, _is_tensor, _like, _p64, _stream_ptr, torch
from .entries import _out_device, submatrices
from .matrices import (AbstractBlockMatrix, BlockSparseMatrix, SymmetricBlockMatrix, _no_mixed_update, _operator, _unwrap, mul, size,
                       update_blocks)

__all__ = ["invert_blocks", "BlockJacobi", "block_jacobi", "Gmres", "GmresInfo", "gmres", "krylov_orth", "krylov_orth_work", "Cg",
           "CgInfo", "cg", "cocg", "BiCgStab", "bicgstab", "GmresMulti"]


# ---- block-Jacobi: the self-interaction blocks inverted where they are (bsm_invert_blocks) -----------------------------
def _square_blocks(blocks):
    """the operand rules of invert_blocks / eigh_blocks: square blocks of ONE element type and device, worked on where they
    are -> _BlockList with the pointers of empty blocks NULL"""
    blocks = list(blocks)
    if _is_dev(blocks):
        kind = _blocks_kind(blocks)
    else:  # host blocks are worked on where they are: none may need a conversion
        dt = None
        for b in blocks:
            if not (isinstance(b, np.ndarray) and b.ndim == 2 and b.dtype in _DT and b.flags.f_contiguous and b.flags.writeable):
                raise TypeError("host blocks must be writeable 2-D Fortran-order numpy arrays of a supported element type")
            if dt is not None and b.dtype != dt:
                raise TypeError("the blocks must share one element type")
            dt = b.dtype
        kind = (dt, False)
    bl = _BlockList(blocks, kind)
    bad = np.nonzero(bl.m != bl.n)[0]
    if len(bad):
        raise ValueError(f"a block of shape {tuple(blocks[bad[0]].shape)} is not square")
    for k in np.nonzero(bl.m == 0)[0]:
        bl.ptrs[k] = None
    return bl


def invert_blocks(blocks):
    """Inverts square column-major blocks IN PLACE (bsm_invert_blocks: Gauss-Jordan with partial row pivoting, one
    workgroup per block on the device, the same elimination serially for host blocks) -> info, one int64 per block:
    0, or the 1-based step whose pivot was zero or not finite (that block is then unspecified).  blocks: numpy arrays
    (Fortran order) or torch CUDA tensors (column-major, e.g. what submatrices(..., device=True) returns) of ONE
    element type and device, orders 0 .. 1024.  Device blocks go on torch's current stream; the call is synchronous."""
    bl = _square_blocks(blocks)
    info = np.zeros(max(len(bl), 1), dtype=np.int64)
    if len(bl) == 0:
        return info[:0]
    st = _stream_ptr(None, bl.blocks[0].device) if bl.dev else None
    L.check(L.lib().bsm_invert_blocks(_DT[bl.dtype], *bl.square_args(), _p64(info), bl.memspace, st))
    return info


# ---- spectral forms of the blocks: eigh_blocks, spectral_blocks (bsm_eigh_blocks, bsm_spectral_blocks) ------------------
_SPEC = {"values": L.BSM_SPEC_VALUES, "inv": L.BSM_SPEC_INV, "absinv": L.BSM_SPEC_ABSINV, "pinv": L.BSM_SPEC_PINV}


def _real_of(dt):
    return np.dtype(np.float32) if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.dtype(np.float64)


def _value_ptrs(ws, bl):
    """the addresses of the eigenvalue arrays of the blocks of bl (NULL for an empty block), each checked: n reals of the
    blocks' precision, contiguous, where the blocks live"""
    real = _real_of(bl.dtype)
    out = (C.c_void_p * max(len(bl), 1))()
    if len(ws) != len(bl):
        raise ValueError(f"{len(ws)} eigenvalue arrays for {len(bl)} blocks")
    for k, (w, n) in enumerate(zip(ws, bl.m)):
        if bl.dev:
            ok = _is_tensor(w) and w.is_cuda and w.device == bl.blocks[k].device and w.dim() == 1 and w.numel() == n and \
                w.dtype == _TORCH_OF[real] and w.is_contiguous()
        else:
            ok = isinstance(w, np.ndarray) and w.ndim == 1 and w.shape[0] == n and w.dtype == real and w.flags.c_contiguous
        if not ok:
            raise TypeError(f"w[{k}] must be a contiguous 1-D {real} array of {int(n)} entries where the blocks live")
        out[k] = None if n == 0 else (w.data_ptr() if bl.dev else w.ctypes.data)
    return out


def eigh_blocks(blocks, vectors=True, *, sweeps=False):
    """Eigendecomposition of square HERMITIAN column-major blocks IN PLACE (bsm_eigh_blocks: two-sided round-robin Jacobi in
    the blocks' own type, one workgroup per block on the device, the same rotations serially for host blocks) -> (w, info):
    w[b] the eigenvalues of (B_b + B_b^H) / 2 ascending -- 1-D real arrays, views of one flat numpy array or of one flat
    tensor on the blocks' device --, block b its orthonormal eigenvectors as columns (vectors=False: unspecified contents);
    info[b] = 0, 1 (a non-finite entry: the block is untouched, w[b] is NaN) or 2 (the cap of 60 sweeps was hit).  The
    operand rules are those of invert_blocks, orders 0 .. 512.  sweeps=True: -> (w, info, sweeps taken per block)."""
    bl = _square_blocks(blocks)
    real = _real_of(bl.dtype)
    info = np.zeros(max(len(bl), 1), dtype=np.int64)
    nsw = np.zeros(max(len(bl), 1), dtype=np.int32)
    off = np.concatenate(([0], np.cumsum(bl.m))).astype(np.int64)
    if bl.dev:
        flat = torch.empty(int(off[-1]), dtype=_TORCH_OF[real], device=bl.blocks[0].device)
    else:
        flat = np.empty(int(off[-1]), dtype=real)
    w = [flat[int(off[k]):int(off[k + 1])] for k in range(len(bl))]
    if len(bl):
        st = _stream_ptr(None, bl.blocks[0].device) if bl.dev else None
        L.check(L.lib().bsm_eigh_blocks(_DT[bl.dtype], *bl.square_args(), _value_ptrs(w, bl), 1 if vectors else 0, _p64(info),
                                        nsw.ctypes.data_as(C.POINTER(C.c_int32)), bl.memspace, st))
    info, nsw = info[:len(bl)], nsw[:len(bl)]
    return (w, info, nsw) if sweeps else (w, info)


def spectral_blocks(V, w, func="inv", rcond=0.0, out=None):
    """out[b] = V[b] diag(f(w[b])) V[b]^H (bsm_spectral_blocks) -> (out, info).  func: "values" (f = w), "inv" (1 / w), "absinv"
    (1 / max(|w|, rcond * max|w|): positive definite) or "pinv" (1 / w where |w| > rcond * max|w|, else 0).  V: square
    column-major blocks as eigh_blocks leaves them, w: its eigenvalue arrays; out: None (fresh blocks like V) or blocks of the
    same kind that overlap neither V nor w.  Hermitian to the bit.  info[b] = 0, or the 1-based index of the first eigenvalue
    at which f is undefined (out[b] is then not written)."""
    if func not in _SPEC:
        raise ValueError(f"func={func!r}: one of {sorted(_SPEC)}")
    bl = _square_blocks(V)
    if out is None:
        if bl.dev:
            out = [torch.empty((int(n), int(n)), dtype=b.dtype, device=b.device).t() for b, n in zip(bl.blocks, bl.m)]
        else:
            out = [np.empty((int(n), int(n)), dtype=bl.dtype, order="F") for n in bl.m]
    ol = _square_blocks(out)
    if (ol.dtype, ol.dev) != (bl.dtype, bl.dev) or len(ol) != len(bl) or np.any(ol.m != bl.m):
        raise ValueError("out must hold blocks of the orders, element type and memory space of V")
    info = np.zeros(max(len(bl), 1), dtype=np.int64)
    if len(bl):
        st = _stream_ptr(None, bl.blocks[0].device) if bl.dev else None
        L.check(L.spectral_blocks_call(_DT[bl.dtype], len(bl), bl.ptrs, _p64(bl.m), _p64(bl.ld), _value_ptrs(list(w), bl), _SPEC[func],
                                       float(rcond), ol.ptrs, _p64(ol.ld), _p64(info), bl.memspace, st))
    return list(out), info[:len(bl)]


def _block_stream(A, stream):
    """-> (whether A's image lives on a device, the context in which submatrices and the block calls take `stream`)"""
    base, _ = _unwrap(A)
    on_dev = base.device is not None or base.devices is not None
    ctx = contextlib.nullcontext()
    if on_dev and stream is not None:
        st = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(stream)
        ctx = torch.cuda.stream(st)  # submatrices and the block calls all take torch's current stream
    return on_dev, ctx


def _inverted_blocks(A, sets, stream=None):
    """[inv(A[I_s, I_s]) for s]: extracted where the image lives and inverted there (device tensors on the handle's first
    device, numpy arrays for an analysis-only handle)"""
    on_dev, ctx = _block_stream(A, stream)
    with ctx:
        blocks = submatrices(A, sets, device=on_dev)
        info = invert_blocks(blocks)
    bad = np.nonzero(info)[0]
    if len(bad):
        raise np.linalg.LinAlgError(f"block_jacobi: A[I, I] of set {int(bad[0]) + 1} is singular to working precision (the pivot of "
                                    f"elimination step {int(info[bad[0]])} is zero or not finite)")
    return blocks


def _spectral_jacobi_blocks(A, sets, kind, rcond, stream=None):
    """([V_s f(w_s) V_s^H for s], [w_s for s]) of A[I_s, I_s] = V_s diag(w_s) V_s^H, f = 1 / |w| (kind "abs") or the pseudo-
    inverse (kind "pinv"): extracted, decomposed and put together where the image lives"""
    on_dev, ctx = _block_stream(A, stream)
    with ctx:
        blocks = submatrices(A, sets, device=on_dev)
        w, info = eigh_blocks(blocks)
        bad = np.nonzero(info)[0]
        if len(bad):
            why = "holds an entry that is not finite" if info[bad[0]] == 1 else "did not converge in the sweep cap of the Jacobi method"
            raise np.linalg.LinAlgError(f"block_jacobi: A[I, I] of set {int(bad[0]) + 1} {why}")
        if kind == "abs" and rcond == 0 and len(w):
            # an eigenvalue the decomposition cannot tell from zero counts as zero: eigh_blocks leaves an exact zero within
            # 4 n eps ||A_ss||_F <= 4 n^1.5 eps max|w| (the accuracy its suite holds it to), and 1 / |w| of such a value is noise
            flat = (torch.cat(w).cpu().numpy() if _is_tensor(w[0]) else np.concatenate(w)).astype(np.float64)
            at, eps = 0, float(np.finfo(_real_of(blocks[0].cpu().numpy().dtype if _is_tensor(blocks[0]) else blocks[0].dtype)).eps)
            for s, ws in enumerate(w):
                n = len(ws)
                mag = np.abs(flat[at:at + n])
                at += n
                small = np.nonzero(mag <= 4 * n ** 1.5 * eps * np.max(mag, initial=0.0))[0] if np.all(np.isfinite(mag)) else []
                if len(small):
                    raise np.linalg.LinAlgError(f"block_jacobi: eigenvalue {int(small[0]) + 1} of A[I, I] of set {s + 1} is zero to working "
                                                f"precision (kind='abs', rcond=0: pass rcond > 0 to clamp, or kind='pinv')")
        out, info = spectral_blocks(blocks, w, "absinv" if kind == "abs" else "pinv", rcond)
    bad = np.nonzero(info)[0]
    if len(bad):
        raise np.linalg.LinAlgError(f"block_jacobi: eigenvalue {int(info[bad[0]])} of A[I, I] of set {int(bad[0]) + 1} is zero or not finite "
                                    f"(kind={kind!r}, rcond={rcond})")
    return out, w


_KINDS = ("inverse", "abs", "pinv")


class BlockJacobi(BlockSparseMatrix):
    """M = sum_s E_s inv(A[I_s, I_s]) E_s^T -- the block-Jacobi (near-field) preconditioner of A as an ordinary
    BlockSparseMatrix handle: mul, M @ X, MulPlan, the wrappers, complex vectors under a real M and M[I, J] work as on
    any other.  Built by block_jacobi(A, sets).  Fields beside BlockSparseMatrix's: `sets` (1-based index arrays),
    `source` (the A it was built from), `kind` ("inverse", "abs" or "pinv": what stands in the place of inv), `rcond` (None
    for "inverse") and `eigenvalues` (None for "inverse"; else the eigenvalues of every A[I_s, I_s] ascending, where the
    blocks live: the inertia of the diagonal blocks)."""

    def __init__(self, A, sets=None, *, kind="inverse", rcond=None, storage=None, accumulate="auto", transpose_image=False):
        base, _ = _operator(A)
        if kind not in _KINDS:
            raise ValueError(f"kind={kind!r}: one of {_KINDS}")
        if kind == "inverse" and rcond is not None:
            raise ValueError("rcond has no meaning with kind='inverse'")
        if rcond is not None and not float(rcond) >= 0:
            raise ValueError(f"rcond={rcond} is negative or NaN")
        if sets is None:
            if not isinstance(base, SymmetricBlockMatrix):
                raise ValueError("sets=None means the diagonalindices of a SymmetricBlockMatrix; pass index sets for other types")
            sets = base.diagonalindices
        m, n = size(A)
        if m != n:
            raise ValueError(f"block_jacobi needs a square operator, size(A) = {(m, n)}")
        self.sets = [_i64(np.asarray(s).reshape(-1)) for s in sets]
        self.source = A
        self.kind = kind
        self.rcond = None if rcond is None else float(rcond)
        blocks, self.eigenvalues = self._build(A)
        dev = L.BSM_DEVICE_NONE if base.device is None and base.devices is None else _out_device(base).index
        super().__init__(blocks, self.sets, self.sets, (m, n), device=dev, storage=storage, accumulate=accumulate,
                         transpose_image=transpose_image)

    def _build(self, A, stream=None):
        """-> (the blocks of M, the eigenvalues or None) from the present values of A, by `kind`"""
        if self.kind == "inverse":
            return _inverted_blocks(A, self.sets, stream), None
        if self.rcond is None:  # (the blocks come in A's vector type: a mixed-storage A gives them widened)
            self.rcond = 0.0 if self.kind == "abs" else float(np.sqrt(np.finfo(_real_of(_unwrap(A)[0].dtype)).eps))
        return _spectral_jacobi_blocks(A, self.sets, self.kind, self.rcond, stream)

    def refresh(self, A=None, stream=None):
        """Re-extracts the blocks of A (default: `source`, e.g. after update_blocks(A, ...)), rebuilds them by the same `kind`
        and pushes them into this handle with update_blocks: no analysis, no reallocation of the image, the tensors of
        `blocks` stay.  A block that raises LinAlgError leaves M (and `eigenvalues`) as it was; a `storage=` M raises what
        update_blocks raises."""
        _no_mixed_update(self)
        A = self.source if A is None else A
        if size(A) != self.size:
            raise ValueError(f"size(A) = {size(A)} but the preconditioner is {self.size}")
        blocks, w = self._build(A, stream)
        update_blocks(self, blocks, stream=stream)
        self.source, self.eigenvalues = A, w


def block_jacobi(A, sets=None, *, kind="inverse", rcond=None, storage=None, accumulate="auto", transpose_image=False):
    """The block-Jacobi preconditioner of A over `sets` (1-based index lists, pairwise disjoint and free of repeats;
    None: the diagonalindices of a SymmetricBlockMatrix) -> BlockJacobi.  submatrices(A, sets, device=True), invert_blocks
    and the BlockSparseMatrix constructor from device tensors: no matrix byte crosses PCIe.  An analysis-only A takes
    the same route on the host and gives an analysis-only M; a multi-device A gives a single-device M on its first
    device; transpose(A) / adjoint(A) are taken as such; a mixed-storage A gives its stored values widened, inverted in
    the vector type (storage= here is that of M).  Rows in no set are zero rows of M -- pass singleton sets for
    point-Jacobi rows.  A singular block raises numpy.linalg.LinAlgError naming the set and the elimination step.

    kind: what M holds for every set, with A[I_s, I_s] = V diag(w) V^H (the caller asserts that these blocks are Hermitian;
    what is decomposed is (A_ss + A_ss^H) / 2 -- eigh_blocks, spectral_blocks in the place of invert_blocks):
      "inverse"  the explicit inverse, as above (rcond must be None);
      "abs"      V diag(1 / |w|) V^H: Hermitian POSITIVE DEFINITE for an indefinite A -- what Minres, Lobpcg and Cg ask of M --
                 and the exact inverse wherever A_ss is definite.  rcond (default 0): |w| is clamped from below at rcond *
                 max|w| of its block.  A zero or non-finite eigenvalue raises LinAlgError naming the set and the eigenvalue's
                 index; with rcond > 0 finite data never raises;
      "pinv"     the Hermitian pseudo-inverse: 1 / w where |w| > rcond * max|w|, else 0, for singular blocks (a floating sub-
                 domain, a pure Neumann patch).  rcond defaults to sqrt(eps) of the type: a regularisation parameter, and a
                 conservative one -- eigenvalues below it are treated as zero.  Never raises for finite data.
    The eigenvalues stay in M.eigenvalues."""
    return BlockJacobi(A, sets, kind=kind, rcond=rcond, storage=storage, accumulate=accumulate, transpose_image=transpose_image)


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


def _copy_guess(X, X0):
    """the initial guess X0 (torch tensor or numpy array, checked) into X, where the solver reads and overwrites it"""
    if X0 is X:
        return
    if _is_tensor(X):
        X.copy_(X0 if isinstance(X0, torch.Tensor) else torch.from_numpy(X0))
    else:
        X[...] = X0.cpu().numpy() if _is_tensor(X0) else X0


class _Solver:
    """What the solver objects share: the checks and the create call (_create), the destroy call, and the prelude of solve().
    A subclass names its entry points in _abi (_abi + "_create" / "_solve" / "_destroy") and calls _create()."""

    _abi = None
    _names = ("B", "X")  # what solve() calls its operands
    _matrices = True  # solve() takes matrices of 1 .. self.nrhs columns beside vectors
    _x0_refusal = "X0 must have the shape {shape} and the type {dtype}"
    _takes_m = True  # the create call has the (M, opM) pair behind (A, opA)

    def _create(self, A, M, dtype, args):
        """the checks and the create call; args(): called once A, M and dtype have passed, gives the arguments of create
        between the vector type and out"""
        base, op = _operator(A)
        mbase, mop = (None, L.BSM_OP_N) if M is None else _operator(M, "M")
        self.dtype = np.dtype(base.dtype if dtype is None else dtype)
        if self.dtype not in _DT:
            raise TypeError(f"dtype={self.dtype} is not a supported vector type")
        args = args()
        self.A, self.M = A, M
        self.nb, self.n = size(A)  # rows of B, rows of X: one number for the solvers of square systems
        self._base, self._mbase = base, mbase
        ptr = C.c_void_p()
        pair = (None if mbase is None else mbase._h.ptr, mop) if self._takes_m else ()
        L.check(getattr(L.lib(), self._abi + "_create")(base._h.ptr, op, *pair, _DT[self.dtype], *args, C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr:
                getattr(L.lib(), self._abi + "_destroy")(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def _prelude(self, B, X, X0, stream):
        """What solve() begins with: B checked, X made like B (None) and checked against it, the guess X0 checked and copied
        into X, the stream settled -> (X, the descriptors of B and of X (_describe), the stream pointer or None)."""
        nb, nx = self._names
        vector = not self._matrices or getattr(B, "ndim", 1) == 1
        b = _describe(B, self.dtype, self.nb, nb, self._base, not vector)
        if X is None:
            X = _like(B, self.n, None if vector else b[2])
        x = _describe(X, self.dtype, self.n, nx, self._base, not vector)
        if x[2] != b[2]:
            raise ValueError(f"DimensionMismatch: {nb} and {nx} have different numbers of columns")
        if b[3] != x[3]:
            raise ValueError(f"{nb} and {nx} must live in the same memory space")
        if self._matrices and not 1 <= b[2] <= self.nrhs:
            raise ValueError(f"{nb} has {b[2]} columns; this solver takes 1 .. {self.nrhs}")
        if X0 is not None:
            if _elt(X0) != self.dtype or tuple(X0.shape) != tuple(X.shape):
                raise TypeError(self._x0_refusal.format(n=self.n, shape=tuple(X.shape), dtype=self.dtype))
            _copy_guess(X, X0)
        st = None
        if b[3] == L.BSM_MEM_DEVICE:
            st = _stream_ptr(stream, B.device)
            if stream is not None and X0 is not None and X0 is not X:
                torch.cuda.current_stream(B.device).synchronize()  # the copy of X0 went on torch's current stream
        return X, b, x, st


class Gmres(_Solver):
    """Right-preconditioned restarted GMRES(restart) for A x = b, every step of it on the device (bsm_gmres_*: the
    solver of GmresMulti with one column behind its own info).
    A: a block matrix or transpose(A) / adjoint(A); M: a preconditioner of the same kind and order (e.g. block_jacobi(A,
    sets)), or None.  dtype: the type of b and x -- default A's vector type; a real A (and M) of the same precision
    takes complex vectors.  The workspace (restart + 3 vectors, restart + 4 with M) is allocated here, once; A and M are
    kept alive."""

    _abi = "bsm_gmres"
    _names = ("b", "x")
    _matrices = False
    _x0_refusal = "x0 must be a vector of {n} entries of {dtype}"

    def __init__(self, A, M=None, restart=30, dtype=None):
        self._create(A, M, dtype, lambda: (int(restart),))
        self.restart = int(restart)

    def solve(self, b, x=None, x0=None, rtol=1e-8, atol=0.0, maxiter=None, stream=None):
        """-> (x, GmresInfo).  b: torch CUDA tensor (enqueued on `stream`, default torch's current stream) or numpy
        array (staged); x: where the solution goes (default: a new vector like b); x0: the initial guess (copied into x;
        None: zero).  Converged when the estimate is <= max(rtol * ||b||, atol); maxiter (default: the order of A)
        bounds the iterations.  Synchronous."""
        x, (bp, _, _, bms, _, _), (xp, *_), st = self._prelude(b, x, x0, stream)
        maxiter = max(self.n, 1) if maxiter is None else int(maxiter)
        hist = np.zeros(max(maxiter, 1), dtype=np.float64)
        p = L.BsmGmresParams(C.sizeof(L.BsmGmresParams), 0 if x0 is None else 1, float(rtol), float(atol), maxiter, maxiter)
        info = L.BsmGmresInfo()
        L.check(L.lib().bsm_gmres_solve(self._ptr, bp, xp, C.byref(p), C.byref(info), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                        bms, st))
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


class _LockstepSolver(_Solver):
    """The solve() of the lockstep solver objects (Cg, BiCgStab, GmresMulti), whose create calls take nrhs_max first."""

    history_capacity = 4096  # rows of CgInfo.history a solve keeps at the most (an attribute: set it on the solver to change it)

    def _setup(self, A, M, nrhs, dtype, extra=lambda: ()):
        """extra(): called once A, M and dtype have passed, gives the arguments of create between nrhs_max and out"""
        self._create(A, M, dtype, lambda: (int(nrhs), *extra()))
        self.nrhs = int(nrhs)

    def solve(self, B, X=None, X0=None, rtol=1e-8, atol=0.0, maxiter=None, stream=None, history=True):
        """-> (X, CgInfo).  B: a vector (n,) or a column-major matrix (n, k), k <= nrhs -- torch CUDA tensor (enqueued on
        `stream`, default torch's current stream) or numpy array (staged), taken as mul takes them; X: where the solution
        goes (default: new, like B); X0: the initial guess (copied into X; None: zero).  Column c is converged when its
        residual norm is <= max(rtol * ||b_c||, atol); maxiter (default: the order of A) bounds the lockstep iterations.
        A vector in gives a vector out.  info.history holds the first min(iterations, history_capacity = 4096) rows;
        history=False keeps none.  Synchronous."""
        X, (bp, ldb, k, bms, _, _), (xp, ldx, *_), st = self._prelude(B, X, X0, stream)
        maxiter = max(self.n, 1) if maxiter is None else int(maxiter)
        cap = min(maxiter, self.history_capacity) if history else 0
        hist = np.empty((max(cap, 1), k), dtype=np.float64)
        p = L.BsmCgParams(C.sizeof(L.BsmCgParams), 0 if X0 is None else 1, float(rtol), float(atol), maxiter, cap)
        info = L.BsmCgInfo()
        cols = (L.BsmCgColumn * k)()
        L.check(getattr(L.lib(), self._abi + "_solve")(self._ptr, k, bp, ldb, xp, ldx, C.byref(p), C.byref(info), cols,
                                                       hist.ctypes.data_as(C.POINTER(C.c_double)), bms, st))
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


# ---- MINRES on several right-hand sides in lockstep, on the device (bsm_minres_*) -------------------------------------------
# (Minres and minres are exported by the package by name, __init__.py: the set of names a star-import gives is pinned by
# tests/test_marshalling_cpu.py and stays as it was)
class Minres(_LockstepSolver):
    """Symmetric-preconditioned MINRES for A X = B with A real symmetric / Hermitian and NOT necessarily definite, and up to
    `nrhs` right-hand sides advancing in lockstep on ONE multi-column product per iteration, every step on the device
    (bsm_minres_*).  The CALLER asserts the symmetry of A, and that M is symmetric / Hermitian POSITIVE definite (e.g.
    block_jacobi of a definite sibling of A); an indefinite M ends a column with status 3.  A: a block matrix or
    transpose(A) / adjoint(A); M: a preconditioner of the same kind and order, or None.  dtype: the type of B and X --
    default A's vector type; a real A (and M) of the same precision takes complex vectors.  The workspace (7 n x nrhs
    matrices, 9 with M) is allocated here, once; A and M are kept alive.  solve() is the one Cg has: the same arguments,
    (X, CgInfo) back; the residual norms are those of the carried residual b - A x in the 2-norm (without M they never grow; with M
    MINRES minimises the M-norm and the 2-norm may rise from one iteration to the next).
    info.a_products = iterations (+ 1 with X0), m_products = iterations + 1 with M."""

    _abi = "bsm_minres"

    def __init__(self, A, M=None, nrhs=1, dtype=None):
        self._setup(A, M, nrhs, dtype)


def minres(A, B, M=None, **kw):
    """One-shot form: Minres(A, M, columns of B, dtype of B).solve(B, **kw) -> (X, info)."""
    k = 1 if getattr(B, "ndim", 1) == 1 else B.shape[1]
    return Minres(A, M, nrhs=k, dtype=_elt(B)).solve(B, **kw)


# ---- LSQR on several right-hand sides in lockstep, on the device (bsm_lsqr_*) -----------------------------------------------
# (Lsqr, LsqrInfo and lsqr are exported by the package by name, like Minres)
class LsqrInfo(CgInfo):
    """CgInfo plus, per column as numpy arrays of k entries: normal_residual (the estimate of ||op(A)^H r - damp^2 (x - x0)||
    when the column stopped) and anorm (the running Frobenius-norm estimate of the bidiagonal factor, scipy's anorm).
    residual and history hold the estimate rnorm of ||b - op(A) x|| (with damp: of the damped residual)."""

    def __init__(self, info, cols, history, normal_residual, anorm):
        super().__init__(info, cols, history)
        self.normal_residual, self.anorm = normal_residual, anorm

    def __repr__(self):
        return "Lsqr" + super().__repr__()[2:]


class Lsqr(_LockstepSolver):
    """LSQR for min ||B - A X||^2 + damp^2 ||X - X0||^2 with A of ANY shape and rank -- over-determined, under-determined
    (the minimum-norm solution) or singular --, up to `nrhs` right-hand sides advancing in lockstep on TWO multi-column
    products per iteration, one with A and one with its adjoint, every step on the device (bsm_lsqr_*).  A: a block matrix
    or transpose(A) / adjoint(A) (transpose of a COMPLEX matrix is refused: its adjoint is conj(A), which no product
    offers); there is no preconditioner argument.  dtype: the type of B and X -- default A's vector type; a real A of the
    same precision takes complex vectors.  B has size(A)[0] rows, X size(A)[1].  The workspace (4 matrices of X's shape, 2
    of B's) is allocated here, once; A is kept alive.  info.a_products = 2 * iterations + 1 (+ 1 with X0)."""

    _abi = "bsm_lsqr"
    _takes_m = False

    def __init__(self, A, nrhs=1, dtype=None):
        self._setup(A, None, nrhs, dtype)

    def solve(self, B, X=None, X0=None, rtol=1e-8, atol=0.0, ntol=1e-8, damp=0.0, maxiter=None, stream=None, history=True):
        """-> (X, LsqrInfo).  B: a vector (m,) or a column-major matrix (m, k), k <= nrhs, m = size(A)[0] -- torch CUDA tensor
        or numpy array, as in Cg.solve; X: where the solution goes (n = size(A)[1] rows; default: new, like B); X0: the
        initial guess (copied into X; None: zero), which is also what damp pulls towards.  Column c stops with status 0
        when the estimate of ||b_c - A x_c|| is <= max(rtol * ||b_c||, atol) (a consistent system), when the estimate of
        the normal-equation residual is <= ntol * anorm * that residual estimate (a least-squares solution), or when the
        Krylov space ends; maxiter (default: min(m, n)) bounds the lockstep iterations.  A vector in gives a vector out.
        Synchronous."""
        X, (bp, ldb, k, bms, _, _), (xp, ldx, *_), st = self._prelude(B, X, X0, stream)
        maxiter = max(min(self.nb, self.n), 1) if maxiter is None else int(maxiter)
        cap = min(maxiter, self.history_capacity) if history else 0
        hist = np.empty((max(cap, 1), k), dtype=np.float64)
        p = L.BsmLsqrParams(C.sizeof(L.BsmLsqrParams), 0 if X0 is None else 1, float(rtol), float(atol), float(ntol), float(damp),
                            maxiter, cap)
        info = L.BsmCgInfo()
        cols = (L.BsmCgColumn * k)()
        arn, an = np.zeros(k), np.zeros(k)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().bsm_lsqr_solve(self._ptr, k, bp, ldb, xp, ldx, C.byref(p), C.byref(info), cols, hist.ctypes.data_as(dp),
                                       arn.ctypes.data_as(dp), an.ctypes.data_as(dp), bms, st))
        return X, LsqrInfo(info, cols, hist[:min(info.iterations, cap)].copy(), arn, an)


def lsqr(A, B, **kw):
    """One-shot form: Lsqr(A, columns of B, dtype of B).solve(B, **kw) -> (X, info)."""
    k = 1 if getattr(B, "ndim", 1) == 1 else B.shape[1]
    return Lsqr(A, nrhs=k, dtype=_elt(B)).solve(B, **kw)


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


# ---- polynomial preconditioners as handles (bsm_poly_*) ---------------------------------------------------------------------
# (PolynomialPreconditioner, polynomial, chebyshev, neumann, chebyshev_coefficients and lanczos_bounds are exported by the
# package by name, like Minres)
def chebyshev_coefficients(lmin, lmax, steps):
    """-> (a, b), float64 arrays of `steps` entries: the coefficients of bsm_poly_create's recurrence for the Chebyshev
    polynomial of a spectrum inside [lmin, lmax] (Saad, Iterative Methods for Sparse Linear Systems, Alg. 12.1):
    theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta, rho_0 = 1 / sigma, b_0 = 1 / theta,
    rho_{k+1} = 1 / (2 sigma - rho_k), a_{k+1} = rho_{k+1} rho_k, b_{k+1} = 2 rho_{k+1} / delta; a_0 = 0 (ignored).  The residual
    polynomial 1 - lambda p(lambda) is T_s((theta - lambda) / delta) / T_s(sigma).  Pure numpy; ValueError unless
    0 < lmin < lmax and steps >= 1."""
    lmin, lmax, steps = float(lmin), float(lmax), int(steps)
    if not (0 < lmin < lmax and np.isfinite(lmax)) or steps < 1:
        raise ValueError(f"chebyshev_coefficients needs 0 < lmin < lmax and steps >= 1, got ({lmin}, {lmax}, {steps})")
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    a, b = np.zeros(steps), np.zeros(steps)
    rho = 1 / sigma
    b[0] = 1 / theta
    for k in range(1, steps):
        nxt = 1 / (2 * sigma - rho)
        a[k], b[k] = nxt * rho, 2 * nxt / delta
        rho = nxt
    return a, b


class PolynomialPreconditioner(AbstractBlockMatrix):
    """z = p(A) x as a handle of its own (bsm_poly_create): `steps` steps of the recurrence r_0 = x, d_0 = b_0 D r_0,
    r_{k+1} = r_k - A d_k, d_{k+1} = a_{k+1} d_k + b_{k+1} D r_{k+1}, p(A) x = d_0 + .. + d_{steps-1}, with real coefficients
    a, b over an operator A and an optional inner preconditioner D (None: the identity) -- steps - 1 multi-column products
    with A and steps with D per product, the vector work between them in fused kernels.  Every solver takes it as M; mul,
    M @ X, transpose(M) and adjoint(M) apply it to torch CUDA tensors of `dtype` (M @ X also to numpy arrays, staged through
    torch).  It holds HANDLES: update_blocks(A, ...) and D.refresh() are seen by the next product.  One product at a time.
    It has no entries: M[I, J], diag, rowcolvals, update_blocks and value_passes raise BsmError.  Built by polynomial(),
    chebyshev() and neumann().  Fields beside AbstractBlockMatrix's: source (A), inner (D), steps, a, b, nrhs."""

    def __init__(self, A, a, b, D=None, nrhs=16, dtype=None):
        base, op = _operator(A)
        dbase, dop = (None, L.BSM_OP_N) if D is None else _operator(D, "D")
        a, b = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in (a, b))
        if len(a) != len(b) or not 1 <= len(b) <= L.BSM_POLY_MAX_STEPS:
            raise ValueError(f"a and b must have the same length, 1 .. {L.BSM_POLY_MAX_STEPS} steps; got {len(a)} and {len(b)}")
        if not (np.all(np.isfinite(b)) and np.all(np.isfinite(a[1:]))):
            raise ValueError("the coefficients must be finite")
        dt = np.dtype(base.dtype if dtype is None else dtype)
        if dt not in _DT:
            raise TypeError(f"dtype={dt} is not a supported vector type")
        m, n = size(A)
        if m != n:
            raise ValueError(f"a polynomial preconditioner needs a square operator, size(A) = {(m, n)}")
        dp = C.POINTER(C.c_double)
        h = C.c_void_p()
        L.check(L.lib().bsm_poly_create(base._h.ptr, op, None if dbase is None else dbase._h.ptr, dop, _DT[dt], int(nrhs), len(b),
                                        a.ctypes.data_as(dp), b.ctypes.data_as(dp), C.byref(h)))
        self._finish(h, dt, (n, n), base.scheduler, base.device)
        self.source, self.inner, self.steps, self.a, self.b, self.nrhs = A, D, len(b), a, b, int(nrhs)

    def _src(self):
        """update_blocks / refresh: what the library answers for a composed handle"""
        L.check(L.lib().bsm_update_blocks(self._h.ptr, 0, None, None, None, L.BSM_MEM_HOST, None))
        raise L.BsmError("a polynomial preconditioner has no blocks")

    def info(self):
        """-> (steps, a, b, workspace bytes) as the library holds them (bsm_poly_info)"""
        steps, ws = C.c_int32(0), C.c_int64(0)
        a, b = np.zeros(L.BSM_POLY_MAX_STEPS), np.zeros(L.BSM_POLY_MAX_STEPS)
        dp = C.POINTER(C.c_double)
        L.check(L.lib().bsm_poly_info(self._h.ptr, C.byref(steps), a.ctypes.data_as(dp), b.ctypes.data_as(dp), C.byref(ws)))
        return steps.value, a[:steps.value], b[:steps.value], ws.value

    def __matmul__(self, x):
        """M @ X.  The library's product takes device vectors only: numpy operands are staged through torch (synchronous)"""
        if _is_tensor(x):
            return super().__matmul__(x)
        x = np.asarray(x, dtype=self.dtype)
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev).t() if x.ndim == 2 else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        y = super().__matmul__(xd).cpu().numpy()
        return np.asfortranarray(y) if y.ndim == 2 else y

    __mul__ = __matmul__


def polynomial(A, a, b, D=None, nrhs=16, dtype=None):
    """The polynomial preconditioner of A with the coefficient arrays a, b of bsm_poly_create's recurrence (a[0] is ignored)
    over the inner preconditioner D (a block matrix of A's order, e.g. block_jacobi(A, sets), or None) -> PolynomialPreconditioner.
    A, D: block matrices or transpose / adjoint wrappers, single-device, with a device image; nrhs: the columns one pass of
    the recurrence takes (1 .. 16; wider operands run in batches); dtype: the type of the vectors -- default A's vector type;
    a real A (and D) of the same precision serves a complex dtype.  The workspace (4 n x nrhs matrices, 5 with D) is
    allocated here, once; A and D are kept alive."""
    return PolynomialPreconditioner(A, a, b, D, nrhs, dtype)


def chebyshev(A, lmin, lmax, steps, D=None, nrhs=16, dtype=None):
    """The Chebyshev polynomial preconditioner of `steps` steps for a spectrum of D A inside [lmin, lmax]
    (chebyshev_coefficients) -> PolynomialPreconditioner.  For symmetric / Hermitian positive definite A and D, with bounds
    from lanczos_bounds: lo, hi = lanczos_bounds(A, D); M = chebyshev(A, 0.95 * lo, 1.05 * hi, steps, D).  steps = 1 is
    D / theta."""
    return PolynomialPreconditioner(A, *chebyshev_coefficients(lmin, lmax, steps), D, nrhs, dtype)


def neumann(A, omega, steps, D=None, nrhs=16, dtype=None):
    """The Neumann (Richardson) polynomial preconditioner omega sum_{k < steps} (I - omega D A)^k D -> PolynomialPreconditioner:
    a_k = 0, b_k = omega.  It approaches inv(A) as steps grows iff rho(I - omega D A) < 1; A need not be symmetric."""
    steps, omega = int(steps), float(omega)
    if steps < 1 or not np.isfinite(omega):
        raise ValueError(f"neumann needs steps >= 1 and a finite omega, got ({omega}, {steps})")
    return PolynomialPreconditioner(A, np.zeros(steps), np.full(steps, omega), D, nrhs, dtype)


def _lanczos_ritz(apply_a, apply_d, v0, steps, xp):
    """The core of lanczos_bounds on any array module xp with vdot (numpy, torch): `steps` preconditioned-CG recurrences on
    A x = v0 with the preconditioner D -> (smallest, largest) eigenvalue of their tridiagonal matrix, the extreme Ritz values
    of D A.  apply_a(v), apply_d(v): A v and D v as new arrays.  It stops early when the Krylov space ends."""
    def dot(u, v):
        return float(xp.vdot(u, v).real)
    r = v0
    z = apply_d(r)
    p = z
    rz = dot(r, z)
    if not rz > 0:
        raise ValueError("lanczos_bounds: <v0, D v0> must be positive (D positive definite, v0 not zero)")
    rz0 = rz
    diag, off = [], []
    alpha_prev = beta_prev = None
    for j in range(int(steps)):
        q = apply_a(p)
        pq = dot(p, q)
        if not pq > 0:
            break
        alpha = rz / pq
        diag.append(1 / alpha + (beta_prev / alpha_prev if j else 0.0))
        r = r - alpha * q
        z = apply_d(r)
        rzn = dot(r, z)
        if j + 1 == int(steps) or not rzn > 1e-28 * rz0:
            break
        beta = rzn / rz
        off.append(beta ** 0.5 / alpha)
        p = z + beta * p
        rz, alpha_prev, beta_prev = rzn, alpha, beta
    if not diag:
        raise ValueError("lanczos_bounds: <p, A p> must be positive (A positive definite)")
    k = len(diag)
    T = np.diag(diag) + np.diag(off[:k - 1], 1) + np.diag(off[:k - 1], -1)
    ev = np.linalg.eigvalsh(T)
    return float(ev[0]), float(ev[-1])


def lanczos_bounds(A, D=None, steps=20, v0=None, seed=0):
    """-> (lo, hi): the extreme Ritz values of D A for a symmetric / Hermitian positive definite A and D (None: the
    identity), from the tridiagonal matrix of `steps` preconditioned-CG recurrences started at v0 (default: uniform in
    (-1, 1) from numpy's default_rng(seed)).  Set-up code: bsm.mul on torch CUDA vectors plus torch reductions, synchronous.
    Ritz values lie INSIDE the spectrum, lo >= lambda_min and hi <= lambda_max, so widen them before use:
    chebyshev(A, 0.95 * lo, 1.05 * hi, steps, D) is the idiom."""
    base, _ = _operator(A)
    if D is not None:
        _operator(D, "D")
    n = size(A)[0]
    dt = np.dtype(base.dtype)
    if base.device is None:
        raise ValueError("lanczos_bounds needs a single-device operator with a device image")
    dev = torch.device("cuda", base.device)
    if v0 is None:
        v0 = np.random.default_rng(seed).uniform(-1, 1, n).astype(dt)
    v = v0 if _is_tensor(v0) else torch.from_numpy(np.ascontiguousarray(np.asarray(v0, dtype=dt))).to(dev)

    def times(H):
        return lambda x: mul(torch.empty_like(x), H, x)
    return _lanczos_ritz(times(A), (lambda x: x) if D is None else times(D), v, steps, torch)


# ---- extreme eigenpairs of symmetric / Hermitian operators on the device (bsm_eigsh_*) and its building block ---------------
# (Eigsh, EigshInfo, eigsh and krylov_combine are exported by the package by name, like Minres)
_EIGSH_WHICH = {"LA": L.BSM_EIGSH_LA, "SA": L.BSM_EIGSH_SA, "BE": L.BSM_EIGSH_BE, "LM": L.BSM_EIGSH_LM}


def krylov_combine_tile(dtype, m):
    """Rows (elements of `dtype`) of the tile one workgroup of krylov_combine stages for m columns (bsm_krylov_combine_tile)."""
    return int(L.lib().bsm_krylov_combine_tile(_DT[np.dtype(dtype)], int(m)))


def krylov_combine(V, S, out=None, carry=None, stream=None):
    """out[:, c] = sum_j V[:, j] S[j, c] on the device (bsm_krylov_combine), the sum over j ascending with one fma per term;
    with carry (a column index of V, 0 .. m) out[:, k] = V[:, carry] too.  V: column-major torch CUDA tensor (n x >= max(m,
    carry + 1)); S: column-major m x k tensor of the REAL type of V's precision (m <= 128, k <= m); out: column-major, n x
    (k, or k + 1 with a carry), of V's type -- None: IN PLACE, the leading columns of V are overwritten and V[:, :k (+ 1)] is
    returned.  out must not overlap V otherwise, and S must not overlap out.  Enqueued on `stream` (default: torch's current stream); nothing is
    synchronised."""
    if torch is None or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (V, S) + (() if out is None else (out,))):
        raise TypeError("krylov_combine takes torch CUDA tensors")
    dt = _TORCH_DT.get(V.dtype)
    if dt is None or V.dim() != 2 or S.dim() != 2:
        raise TypeError("V must be a matrix of a supported element type and S a matrix")
    if _TORCH_DT.get(S.dtype) != np.dtype(np.zeros(1, dt).real.dtype):
        raise TypeError(f"S must have the real type of the precision of {dt}")
    n, (m, k) = V.shape[0], S.shape
    c = -1 if carry is None else int(carry)
    cols = k + (1 if c >= 0 else 0)
    if not (1 <= m <= L.BSM_GMRES_MAX_RESTART and k <= m and -1 <= c <= m and V.shape[1] >= max(m, c + 1)):
        raise ValueError(f"S is {m} x {k}, carry = {carry}: m must be 1 .. {L.BSM_GMRES_MAX_RESTART}, k <= m, carry in 0 .. m, and V hold "
                         "the columns they name")
    if out is None:
        out = V[:, :cols]
    if out.dtype != V.dtype or out.dim() != 2 or tuple(out.shape) != (n, cols) or out.device != V.device or S.device != V.device:
        raise ValueError(f"out must be a {n} x {cols} matrix of V's type on V's device, S live there too")
    for t, name in ((V, "V"), (S, "S"), (out, "out")):
        if t.shape[0] > 1 and t.stride(0) != 1:
            raise TypeError(f"{name} must be column-major (e.g. torch.empty(cols, ld).t()[:n])")

    def ld(t):
        return t.stride(1) if t.shape[1] > 1 else max(t.shape[0], 1)
    L.check(L.lib().bsm_krylov_combine(_DT[dt], n, m, k, V.data_ptr(), ld(V), S.data_ptr(), ld(S), out.data_ptr(),
                                       ld(V) if out.data_ptr() == V.data_ptr() and out.shape[1] <= 1 else ld(out), c,
                                       _stream_ptr(stream, V.device)))
    return out


class EigshInfo:
    """What a solve reports (bsm_eigsh_info and the bsm_eigsh_pair entries): status (0 converged, 1 maxcycles reached, 2 a
    non-finite norm or Ritz value, 3 the Krylov space ended before nev pairs existed), nconv, cycles, a_products (Lanczos
    steps + residual columns), anorm (the largest |Ritz value| seen: a lower bound of ||A||_2), workspace_bytes, workspace;
    per pair, as numpy arrays of nconv entries: value, estimate (|beta_m S[m - 1, i]|), residual (the true
    ||A x - theta x||; the estimate with vectors=False)."""

    def __init__(self, info, pairs):
        for name, _ in L.BsmEigshInfo._fields_:
            if name != "reserved":
                setattr(self, name, getattr(info, name))
        k = self.nconv
        self.value = np.array([pairs[i].value for i in range(k)], dtype=np.float64)
        self.estimate = np.array([pairs[i].estimate for i in range(k)], dtype=np.float64)
        self.residual = np.array([pairs[i].residual for i in range(k)], dtype=np.float64)

    @property
    def converged(self):
        return self.status == 0

    def __repr__(self):
        return (f"EigshInfo(status={self.status}, nconv={self.nconv}, cycles={self.cycles}, a_products={self.a_products}, "
                f"anorm={self.anorm:.3e})")


class Eigsh:
    """`nev` extreme eigenpairs of a real symmetric / complex Hermitian A by thick-restart Lanczos (the Hermitian
    Krylov-Schur method), the basis, the products, the orthogonalisation and the restart on the device (bsm_eigsh_*).  The
    CALLER asserts the symmetry.  A: a block matrix or transpose(A) / adjoint(A), single-device with a device image.  which:
    "LA" (largest algebraic), "SA" (smallest), "BE" (both ends: ceil(nev / 2) from the top, the rest from the bottom), "LM"
    (largest magnitude).  ncv: columns of the basis, nev + 2 .. min(n, 128); default min(n, 128, max(2 nev + 1, 20)).  dtype: A's
    own vector type (a mixed-storage A solves in double).  The workspace (ncv + 1 + min(nev, 16) vectors) is allocated here,
    once; A is kept alive and update_blocks(A, ...) is seen by the next solve.  Not in it: interior eigenvalues,
    shift-invert, the generalised problem, preconditioning, multiplicities, singular values, block methods."""

    def __init__(self, A, nev=6, ncv=None, which="LA", dtype=None):
        base, op = _operator(A)
        self.dtype = np.dtype(base.dtype if dtype is None else dtype)
        if self.dtype not in _DT:
            raise TypeError(f"dtype={self.dtype} is not a supported vector type")
        if which not in _EIGSH_WHICH:
            raise ValueError(f"which={which!r}: 'LA', 'SA', 'BE' or 'LM'")
        m, n = size(A)
        self.nev = int(nev)
        self.ncv = min(n, L.BSM_GMRES_MAX_RESTART, max(2 * self.nev + 1, 20)) if ncv is None else int(ncv)
        self.which, self.A, self.n, self._base = which, A, n, base
        ptr = C.c_void_p()
        L.check(L.lib().bsm_eigsh_create(base._h.ptr, op, _DT[self.dtype], self.nev, self.ncv, C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr:
                L.lib().bsm_eigsh_destroy(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def solve(self, v0=None, rtol=1e-10, atol=0.0, maxcycles=300, vectors=True, stream=None, seed=0, *, X=None):
        """-> (w, X, EigshInfo).  v0: the start vector, n entries -- torch CUDA tensor (the solve is enqueued on `stream`,
        default torch's current stream) or numpy array (staged); None: uniform in (-1, 1) from numpy's default_rng(seed), on
        A's device.  X: where the Ritz vectors go (n x nev, column-major, like v0; None: new); with vectors=False it is not
        touched and (w, None, info) comes back.  w: the info.nconv eigenvalues in the order of `which` (numpy); X[:, :nconv]
        their vectors, orthonormal.  Converged when every wanted pair's estimate is <= max(rtol * anorm, atol).  Synchronous."""
        if v0 is None:
            v0 = np.random.default_rng(seed).uniform(-1, 1, self.n)
            if self.dtype.kind == "c":
                v0 = v0 + 0j
            v0 = torch.from_numpy(v0.astype(self.dtype)).to(torch.device("cuda", self._base.device))
        vp, _, _, ms, _, _ = _describe(v0, self.dtype, self.n, "v0", self._base)
        xp, ldx = None, max(self.n, 1)
        if vectors:
            if X is None:
                X = _like(v0, self.n, self.nev)
            xp, ldx, k, xms, _, _ = _describe(X, self.dtype, self.n, "X", self._base, True)
            if k != self.nev:
                raise ValueError(f"DimensionMismatch: X has {k} columns, expected nev = {self.nev}")
            if xms != ms:
                raise ValueError("v0 and X must live in the same memory space")
        st = _stream_ptr(stream, v0.device) if ms == L.BSM_MEM_DEVICE else None
        p = L.BsmEigshParams(C.sizeof(L.BsmEigshParams), _EIGSH_WHICH[self.which], float(rtol), float(atol), int(maxcycles),
                             1 if vectors else 0)
        info = L.BsmEigshInfo()
        pairs = (L.BsmEigshPair * self.nev)()
        L.check(L.lib().bsm_eigsh_solve(self._ptr, vp, xp, ldx, C.byref(p), C.byref(info), pairs, ms, st))
        out = EigshInfo(info, pairs)
        return out.value.copy(), (X if vectors else None), out


def eigsh(A, nev=6, ncv=None, which="LA", dtype=None, **kw):
    """One-shot form: Eigsh(A, nev, ncv, which, dtype).solve(**kw) -> (w, X, EigshInfo)."""
    return Eigsh(A, nev=nev, ncv=ncv, which=which, dtype=dtype).solve(**kw)


# ---- largest / smallest singular triplets of rectangular operators on the device (bsm_svds_*) --------------------------------
# (Svds, SvdsInfo and svds are exported by the package by name, like Eigsh)
_SVDS_WHICH = {"LM": L.BSM_SVDS_LM, "SM": L.BSM_SVDS_SM}


class SvdsInfo:
    """What a solve reports (bsm_svds_info and the bsm_svds_triplet entries): status (0 converged, 1 maxcycles reached, 2 a
    non-finite norm or value or the sweep cap of the small SVD, 3 the space ended before nsv triplets existed), nconv, cycles,
    a_products (2 x steps + 2 x residual columns), anorm (the largest sigma seen: a lower bound of ||A||_2), workspace_bytes,
    workspace; per triplet, as numpy arrays of nconv entries: value, estimate (|beta_m X[m - 1, i]|), residual_av (the true
    ||A v - sigma u||) and residual_ahu (||A^H u - sigma v||); with vectors=False the estimate stands for the one that belongs
    to the short side's product, zero for the other."""

    def __init__(self, info, triplets):
        for name, _ in L.BsmSvdsInfo._fields_:
            if name != "reserved":
                setattr(self, name, getattr(info, name))
        k = self.nconv
        for f in ("value", "estimate", "residual_av", "residual_ahu"):
            setattr(self, f, np.array([getattr(triplets[i], f) for i in range(k)], dtype=np.float64))

    @property
    def converged(self):
        return self.status == 0

    def __repr__(self):
        return (f"SvdsInfo(status={self.status}, nconv={self.nconv}, cycles={self.cycles}, a_products={self.a_products}, "
                f"anorm={self.anorm:.3e})")


class Svds:
    """The `nsv` largest ("LM") or smallest ("SM") singular triplets of a rectangular or nonsymmetric A (m x n) by thick-restart
    Golub-Kahan-Lanczos bidiagonalisation with full two-sided reorthogonalisation, the bases, both products, the
    orthogonalisation, the restart and the true residuals on the device (bsm_svds_*).  A: a block matrix or transpose(A) /
    adjoint(A) (transpose of a complex A is refused: it would need conj(A)), single-device with a device image.  ncv: columns of
    the bases, nsv + 2 .. min(m, n, 128); default min(m, n, 128, max(2 nsv + 1, 20)).  dtype: A's own vector type (a mixed-storage
    A solves in double).  The workspace (2 ncv + 1 + 2 min(nsv, 16) vectors) is allocated here, once; A is kept alive and
    update_blocks(A, ...) is seen by the next solve.  One product per step is a transposed one: two solves give the same bytes
    only on handles whose transposed product is reproducible (transpose_image=True on a conflict-free operator, gather,
    coloured).  NOT in it: one-sided reorthogonalisation, harmonic / refined Ritz values or shift-invert for interior and tiny
    values, a block method, multi-device and own-range handles, graph capture."""

    def __init__(self, A, nsv=6, ncv=None, which="LM", dtype=None):
        base, op = _operator(A)
        self.dtype = np.dtype(base.dtype if dtype is None else dtype)
        if self.dtype not in _DT:
            raise TypeError(f"dtype={self.dtype} is not a supported vector type")
        if which not in _SVDS_WHICH:
            raise ValueError(f"which={which!r}: 'LM' or 'SM'")
        m, n = size(A)
        self.nsv = int(nsv)
        self.ncv = min(m, n, L.BSM_GMRES_MAX_RESTART, max(2 * self.nsv + 1, 20)) if ncv is None else int(ncv)
        self.which, self.A, self.m, self.n, self._base = which, A, m, n, base
        ptr = C.c_void_p()
        L.check(L.lib().bsm_svds_create(base._h.ptr, op, _DT[self.dtype], self.nsv, self.ncv, C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr:
                L.lib().bsm_svds_destroy(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def solve(self, v0=None, rtol=1e-10, atol=0.0, maxcycles=300, vectors=True, stream=None, seed=0, *, U=None, V=None):
        """-> (s, U, V, SvdsInfo).  v0: the start vector, min(m, n) entries -- torch CUDA tensor (the solve is enqueued on
        `stream`, default torch's current stream) or numpy array (staged); None: uniform in (-1, 1) from numpy's
        default_rng(seed), on A's device.  U (m x nsv), V (n x nsv): where the singular vectors go (column-major, like v0;
        None: new); with vectors=False they are not touched and (s, None, None, info) comes back.  s: the info.nconv singular
        values in the order of `which` (numpy); U[:, :nconv], V[:, :nconv] their vectors, orthonormal, A V = U diag(s).
        Converged when every wanted triplet's estimate is <= max(rtol * anorm, atol).  Synchronous."""
        short = min(self.m, self.n)
        if v0 is None:
            v0 = np.random.default_rng(seed).uniform(-1, 1, short)
            if self.dtype.kind == "c":
                v0 = v0 + 0j
            v0 = torch.from_numpy(v0.astype(self.dtype)).to(torch.device("cuda", self._base.device))
        vp, _, _, ms, _, _ = _describe(v0, self.dtype, short, "v0", self._base)
        up, ldu, wp, ldv = None, max(self.m, 1), None, max(self.n, 1)
        if vectors:
            U = _like(v0, self.m, self.nsv) if U is None else U
            V = _like(v0, self.n, self.nsv) if V is None else V
            up, ldu, ku, ums, _, _ = _describe(U, self.dtype, self.m, "U", self._base, True)
            wp, ldv, kv, vms, _, _ = _describe(V, self.dtype, self.n, "V", self._base, True)
            if ku != self.nsv or kv != self.nsv:
                raise ValueError(f"DimensionMismatch: U, V have {ku}, {kv} columns, expected nsv = {self.nsv}")
            if ums != ms or vms != ms:
                raise ValueError("v0, U and V must live in the same memory space")
        st = _stream_ptr(stream, v0.device) if ms == L.BSM_MEM_DEVICE else None
        p = L.BsmSvdsParams(C.sizeof(L.BsmSvdsParams), _SVDS_WHICH[self.which], float(rtol), float(atol), int(maxcycles),
                            1 if vectors else 0)
        info = L.BsmSvdsInfo()
        trip = (L.BsmSvdsTriplet * self.nsv)()
        L.check(L.lib().bsm_svds_solve(self._ptr, vp, up, ldu, wp, ldv, C.byref(p), C.byref(info), trip, ms, st))
        out = SvdsInfo(info, trip)
        return out.value.copy(), (U if vectors else None), (V if vectors else None), out


def svds(A, nsv=6, ncv=None, which="LM", dtype=None, **kw):
    """One-shot form: Svds(A, nsv, ncv, which, dtype).solve(**kw) -> (s, U, V, SvdsInfo)."""
    return Svds(A, nsv=nsv, ncv=ncv, which=which, dtype=dtype).solve(**kw)


# ---- LOBPCG on the device (bsm_lobpcg_*) and the two tall-skinny products of a block method ---------------------------------
# (Lobpcg, LobpcgInfo, lobpcg, block_gram and block_combine are exported by the package by name, like Eigsh)
def _wide(dt):
    return np.dtype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)


def _ld(t):
    return t.stride(1) if t.shape[1] > 1 else max(t.shape[0], 1)


def _column_major(ts, fn):
    if torch is None or not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 for t, _ in ts):
        raise TypeError(f"{fn} takes torch CUDA matrices")
    for t, name in ts:
        if t.shape[0] > 1 and t.stride(0) != 1:
            raise TypeError(f"{name} must be column-major (e.g. torch.empty(cols, ld).t()[:n])")
        if t.device != ts[0][0].device:
            raise ValueError(f"{name} must live on the device of {ts[0][1]}")


def block_gram_grid(dtype, n):
    """Workgroups (row ranges) of the first launch of block_gram on n rows of `dtype` (bsm_block_gram_grid)."""
    return int(L.lib().bsm_block_gram_grid(_DT[np.dtype(dtype)], int(n)))


def block_gram_work(dtype, n, p, q):
    """Bytes of the work buffer of block_gram (bsm_block_gram_work)."""
    return int(L.lib().bsm_block_gram_work(_DT[np.dtype(dtype)], int(n), int(p), int(q)))


def block_gram(U, W, out=None, stream=None, *, work=None):
    """out = U^H W on the device (bsm_block_gram).  U: n x p (p <= 48), W: n x q (q <= 96), column-major torch CUDA matrices of
    one element type, any alignment; W may alias or contain U.  out: p x q column-major of the WIDE type (float64 / complex128;
    None: new).  work: a 16-byte aligned CUDA tensor of at least block_gram_work(...) bytes (None: new).  Partial sums per row
    range on the matrix pipe in U's precision, added in a fixed order in double: run to run the same bits.  Enqueued on
    `stream` (default: torch's current stream); nothing is synchronised."""
    _column_major([(U, "U"), (W, "W")] + ([] if out is None else [(out, "out")]), "block_gram")
    dt = _TORCH_DT.get(U.dtype)
    if dt is None or W.dtype != U.dtype or U.shape[0] != W.shape[0]:
        raise TypeError("U and W must have one supported element type and the same number of rows")
    n, p, q = U.shape[0], U.shape[1], W.shape[1]
    if not (1 <= p <= 48 and 1 <= q <= 96):
        raise ValueError(f"U has {p} columns and W {q}: 1 .. 48 and 1 .. 96")
    if out is None:
        out = torch.empty((q, p), dtype=_TORCH_OF[_wide(dt)], device=U.device).t()
    if _TORCH_DT.get(out.dtype) != _wide(dt) or tuple(out.shape) != (p, q):
        raise ValueError(f"out must be a {p} x {q} matrix of {_wide(dt)}")
    need = block_gram_work(dt, n, p, q)
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=U.device)
    if work.device != U.device or work.numel() * work.element_size() < need:
        raise ValueError(f"work must hold {need} bytes on U's device")
    L.check(L.lib().bsm_block_gram(_DT[dt], n, p, U.data_ptr(), _ld(U), q, W.data_ptr(), _ld(W), out.data_ptr(), _ld(out),
                                   work.data_ptr(), _stream_ptr(stream, U.device)))
    return out


def block_combine_tile(dtype, p):
    """Rows (elements of `dtype`) of the tile one workgroup of block_combine stages for p columns (bsm_block_combine_tile)."""
    return int(L.lib().bsm_block_combine_tile(_DT[np.dtype(dtype)], int(p)))


def block_combine(V, C, out=None, stream=None):
    """out[:, c] = sum_j V[:, j] C[j, c] on the device (bsm_block_combine), C of V's own type -- complex for complex V --, the sum
    over j ascending with fused multiply-adds: fixed to the bit.  V: n x >= p, C: p x q (p <= 48, q <= p), column-major torch
    CUDA matrices; out: n x q of V's type -- None: IN PLACE, the leading q columns of V are overwritten and returned.  Enqueued
    on `stream` (default: torch's current stream); nothing is synchronised."""
    _column_major([(V, "V"), (C, "C")] + ([] if out is None else [(out, "out")]), "block_combine")
    dt = _TORCH_DT.get(V.dtype)
    if dt is None or C.dtype != V.dtype:
        raise TypeError("V and C must have one supported element type")
    n, (p, q) = V.shape[0], C.shape
    if not (1 <= p <= 48 and q <= p and V.shape[1] >= p):
        raise ValueError(f"C is {p} x {q}: p must be 1 .. 48, q <= p, and V hold p columns")
    if out is None:
        out = V[:, :q]
    if out.dtype != V.dtype or tuple(out.shape) != (n, q):
        raise ValueError(f"out must be a {n} x {q} matrix of V's type")
    L.check(L.lib().bsm_block_combine(_DT[dt], n, p, q, V.data_ptr(), _ld(V), C.data_ptr(), _ld(C), out.data_ptr(),
                                      _ld(V) if out.data_ptr() == V.data_ptr() and out.shape[1] <= 1 else _ld(out),
                                      _stream_ptr(stream, V.device)))
    return out


class LobpcgInfo:
    """What a solve reports (bsm_lobpcg_info and the bsm_eigsh_pair entries): status (0 converged, 1 maxiter reached, 2 a
    non-finite norm, Gram entry or Ritz value, 3 fewer than `block` directions kept), nconv, iterations, drops (directions the
    Rayleigh-Ritz steps dropped), a_products (= iterations + 2 multi-column products), m_products (= iterations), anorm (the
    largest |Ritz value| seen: a lower bound of ||A||_2), workspace_bytes; per pair, as numpy arrays of nev entries: value,
    estimate (the CARRIED residual norm), residual (the true ||A x - theta x||); history: (iterations + 1) x nev carried norms
    (None without history)."""

    def __init__(self, info, pairs, nev, history):
        for name, _ in L.BsmLobpcgInfo._fields_:
            setattr(self, name, getattr(info, name))
        self.value = np.array([pairs[i].value for i in range(nev)], dtype=np.float64)
        self.estimate = np.array([pairs[i].estimate for i in range(nev)], dtype=np.float64)
        self.residual = np.array([pairs[i].residual for i in range(nev)], dtype=np.float64)
        self.history = history

    @property
    def converged(self):
        return self.status == 0

    def __repr__(self):
        return (f"LobpcgInfo(status={self.status}, nconv={self.nconv}, iterations={self.iterations}, drops={self.drops}, "
                f"a_products={self.a_products}, m_products={self.m_products}, anorm={self.anorm:.3e})")


class Lobpcg:
    """The `nev` smallest (which="SA") or largest ("LA") eigenpairs of a real symmetric / complex Hermitian A by LOBPCG on a
    block of `block` vectors (bsm_lobpcg_*), with an optional preconditioner M -- Hermitian positive definite, ~ inv(A) on the
    wanted end: block_jacobi(A), chebyshev(A, ...), neumann(A, ...) or any block matrix.  The CALLER asserts both.  A block
    method finds every copy of a multiple eigenvalue, and A is streamed once per iteration for the whole block.  block: nev ..
    16, 3 block <= n; None: min(16, nev + 2).  dtype: A's own vector type (a mixed-storage A solves in double).  The workspace
    (6 block vectors, 7 with M) is allocated here, once; A and M are kept alive and update_blocks(A, ...) is seen by the next
    solve.  Per iteration the host synchronises once and runs a Rayleigh-Ritz step of order up to 3 block."""

    def __init__(self, A, nev=4, block=None, M=None, which="SA", dtype=None):
        base, op = _operator(A)
        mbase, mop = (None, L.BSM_OP_N) if M is None else _operator(M, "M")
        self.dtype = np.dtype(base.dtype if dtype is None else dtype)
        if self.dtype not in _DT:
            raise TypeError(f"dtype={self.dtype} is not a supported vector type")
        if which not in ("SA", "LA"):
            raise ValueError(f"which={which!r}: 'SA' or 'LA'")
        m, n = size(A)
        self.nev = int(nev)
        self.block = min(L.BSM_CG_MAX_RHS, self.nev + 2) if block is None else int(block)
        self.which, self.A, self.M, self.n, self._base, self._mbase = which, A, M, n, base, mbase
        ptr = C.c_void_p()
        L.check(L.lib().bsm_lobpcg_create(base._h.ptr, op, None if mbase is None else mbase._h.ptr, mop, _DT[self.dtype], self.nev,
                                          self.block, C.byref(ptr)))
        self._ptr = ptr

    def __del__(self):
        try:
            if self._ptr:
                L.lib().bsm_lobpcg_destroy(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def solve(self, X0=None, rtol=1e-10, atol=0.0, maxiter=200, stream=None, seed=0, history=True, *, X=None):
        """-> (w, X, LobpcgInfo).  X0: the start block, n x block, column-major -- torch CUDA tensor (the solve is enqueued on
        `stream`, default torch's current stream) or numpy array (staged); None: uniform in (-1, 1) from numpy's
        default_rng(seed), on A's device.  X: where the vectors go (n x nev, column-major, like X0; None: new).  w: the nev
        eigenvalues in the order of `which` (numpy; NaN with status 2 or 3, X is then not written).  Converged when the carried
        residual norms of the first nev columns are <= max(rtol * anorm, atol).  Synchronous."""
        if X0 is None:
            X0 = np.random.default_rng(seed).uniform(-1, 1, (self.n, self.block))
            if self.dtype.kind == "c":
                X0 = X0 + 0j
            X0 = torch.from_numpy(np.ascontiguousarray(X0.astype(self.dtype).T)).to(torch.device("cuda", self._base.device)).t()
        x0p, ldx0, k0, ms, _, _ = _describe(X0, self.dtype, self.n, "X0", self._base, True)
        if k0 != self.block:
            raise ValueError(f"DimensionMismatch: X0 has {k0} columns, expected block = {self.block}")
        if X is None:
            X = _like(X0, self.n, self.nev)
        xp, ldx, k, xms, _, _ = _describe(X, self.dtype, self.n, "X", self._base, True)
        if k != self.nev:
            raise ValueError(f"DimensionMismatch: X has {k} columns, expected nev = {self.nev}")
        if xms != ms:
            raise ValueError("X0 and X must live in the same memory space")
        st = _stream_ptr(stream, X0.device) if ms == L.BSM_MEM_DEVICE else None
        p = L.BsmLobpcgParams(C.sizeof(L.BsmLobpcgParams), _EIGSH_WHICH[self.which], float(rtol), float(atol), int(maxiter), 0)
        info = L.BsmLobpcgInfo()
        pairs = (L.BsmEigshPair * self.nev)()
        cap = int(maxiter) + 1 if history else 0
        hist = np.full((max(cap, 1), self.nev), np.nan)
        L.check(L.lib().bsm_lobpcg_solve(self._ptr, x0p, ldx0, xp, ldx, C.byref(p), C.byref(info), pairs,
                                         hist.ctypes.data_as(C.POINTER(C.c_double)) if history else None, cap, ms, st))
        out = LobpcgInfo(info, pairs, self.nev, hist[:info.iterations + 1].copy() if history and info.status <= 1 else None)
        return out.value.copy(), X, out


def lobpcg(A, nev=4, block=None, M=None, which="SA", dtype=None, **kw):
    """One-shot form: Lobpcg(A, nev, block, M, which, dtype).solve(**kw) -> (w, X, LobpcgInfo)."""
    return Lobpcg(A, nev=nev, block=block, M=M, which=which, dtype=dtype).solve(**kw)
