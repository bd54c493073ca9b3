"""Argument checks of the Python layer, pinned by exception type and FULL message: the refusals that pass through the
shared marshalling code (block lists, operand descriptors, the solver prelude, the VBCRS sources, the wrapper check).
Everything runs on analysis-only handles.  A solver object needs a device image to exist, so its create and solve entry
points are replaced by stand-ins for the solver cases: every check under test comes before the solve call, which is
never reached.  The device-only forms of these checks are in test_gpu_device_blocks.py."""
import numpy as np
import pytest
import torch

from _common import NODEV

I4 = [[1, 2, 3, 4], [5, 6, 7, 8]]


def _blocks(dtype=np.float64):
    return [np.asfortranarray(np.arange(16).reshape(4, 4) + 4 * np.eye(4), dtype=dtype) for _ in range(2)]


@pytest.fixture(scope="module")
def ops(bsm):
    """one 8 x 8 operator of two 4 x 4 blocks as each storage type, and an operator with no block at all"""
    A = bsm.BlockSparseMatrix(_blocks(), I4, I4, (8, 8), device=NODEV)
    S = bsm.SymmetricBlockMatrix(_blocks(), I4, [np.ones((4, 4))], [I4[0]], [I4[1]], (8, 8), device=NODEV)
    V = bsm.VariableBlockCompressedRowStorage(S, device=NODEV, materialize=True)
    E = bsm.BlockSparseMatrix([], [], [], (8, 8), device=NODEV)
    ES = bsm.SymmetricBlockMatrix([], [], [], [], [], (8, 8), device=NODEV)
    return dict(A=A, S=S, V=V, E=E, ES=ES)


@pytest.fixture
def solvers(bsm, ops, monkeypatch):
    """a Cg of two columns and a Gmres on the analysis-only operator, behind stand-ins for create and solve"""
    lib = bsm._lib.lib()
    for abi in ("bsm_cg", "bsm_gmres"):
        monkeypatch.setattr(lib, abi + "_create", lambda *a: 0)  # leaves the handle NULL, which destroy accepts
        monkeypatch.setattr(lib, abi + "_solve", lambda *a: pytest.fail("a refused solve reached the library"))
    return dict(cg=bsm.Cg(ops["A"], nrhs=2), gmres=bsm.Gmres(ops["A"]))


def z(*shape, dtype=np.float64, order="C"):
    return np.zeros(shape, dtype=dtype, order=order)


def tz(*shape, dtype=torch.float64):
    return torch.zeros(shape, dtype=dtype)


def tf(n, k, dtype=torch.float64):
    """a column-major torch matrix"""
    return torch.zeros((k, n), dtype=dtype).t()


MIXED = ("storage=%s with %s blocks: mixed precision stores float64 blocks as float32 and complex128 blocks as complex64, "
         "nothing else")
MATERIALISED = ("update_blocks / refresh of a VBCRS that materialised a SymmetricBlockMatrix: build it with materialize=False "
                "(the symmetric image, which refreshes from the source's lists)")

# (id, what to call with (bsm, ops, solvers), exception type, full message)
CASES = [
    # ---- vector operands of mul: x before y, dimension before type for torch ------------------------------------------
    ("mul-x-length", lambda b, o, s: b.mul(z(8), o["A"], z(7)), ValueError,
     "DimensionMismatch: x has shape (7,), expected (8,)"),
    ("mul-y-length", lambda b, o, s: b.mul(z(9), o["A"], z(8)), ValueError,
     "DimensionMismatch: y has shape (9,), expected (8,)"),
    ("mul-x-before-y", lambda b, o, s: b.mul(z(9), o["A"], z(7)), ValueError,
     "DimensionMismatch: x has shape (7,), expected (8,)"),
    ("mul-x-dtype", lambda b, o, s: b.mul(z(8), o["A"], z(8, dtype=np.float32)), TypeError,
     "x must be a contiguous float64 array"),
    ("mul-y-strided", lambda b, o, s: b.mul(z(16)[::2], o["A"], z(8)), TypeError,
     "y must be a contiguous float64 array"),
    ("mul-x-list", lambda b, o, s: b.mul(z(8), o["A"], [0.0] * 8), TypeError,
     "x must be a numpy array or a torch tensor"),
    ("mul-x-torch-length", lambda b, o, s: b.mul(tz(8), o["A"], tz(7)), ValueError,
     "DimensionMismatch: x has length (7,), expected 8"),
    ("mul-x-torch-length-before-dtype", lambda b, o, s: b.mul(tz(8), o["A"], tz(7, dtype=torch.float32)), ValueError,
     "DimensionMismatch: x has length (7,), expected 8"),
    ("mul-x-torch-dtype", lambda b, o, s: b.mul(tz(8), o["A"], tz(8, dtype=torch.float32)), TypeError,
     "x must be a contiguous torch.float64 tensor"),
    ("mul-y-torch-strided", lambda b, o, s: b.mul(tz(16)[::2], o["A"], tz(8)), TypeError,
     "y must be a contiguous torch.float64 tensor"),
    ("mul-transpose-lengths", lambda b, o, s: b.mul(z(8), b.transpose(o["A"]), z(7)), ValueError,
     "DimensionMismatch: x has shape (7,), expected (8,)"),
    # ---- matrix operands of mul ---------------------------------------------------------------------------------------------
    ("mul-X-rows", lambda b, o, s: b.mul(z(8, 2, order="F"), o["A"], z(7, 2, order="F")), ValueError,
     "DimensionMismatch: X must be a 2-D array with 8 rows"),
    ("mul-X-vector-under-Y-matrix", lambda b, o, s: b.mul(z(8, 2, order="F"), o["A"], z(8)), ValueError,
     "DimensionMismatch: X must be a 2-D array with 8 rows"),
    ("mul-X-list", lambda b, o, s: b.mul(z(8, 2, order="F"), o["A"], [[0.0, 0.0]] * 8), ValueError,
     "DimensionMismatch: X must be a 2-D array with 8 rows"),
    ("mul-X-order", lambda b, o, s: b.mul(z(8, 2, order="F"), o["A"], z(8, 2)), TypeError,
     "X must be a column-major (Fortran-order) float64 array"),
    ("mul-Y-dtype", lambda b, o, s: b.mul(z(8, 2, dtype=np.complex128, order="F"), o["A"], z(8, 2, order="F")), TypeError,
     "a float64 matrix with x of float64 and y of complex128: supported pairs: (float64, complex128) and (float32, complex64)"),
    ("mul-Y-order", lambda b, o, s: b.mul(z(8, 2), o["A"], z(8, 2, order="F")), TypeError,
     "Y must be a column-major (Fortran-order) float64 array"),
    ("mul-X-torch-rows", lambda b, o, s: b.mul(tf(8, 2), o["A"], tf(7, 2)), ValueError,
     "DimensionMismatch: X has shape (7, 2), expected (8, k)"),
    ("mul-X-torch-rows-before-dtype", lambda b, o, s: b.mul(tf(8, 2), o["A"], tf(7, 2, torch.float32)), ValueError,
     "DimensionMismatch: X has shape (7, 2), expected (8, k)"),
    ("mul-X-torch-order", lambda b, o, s: b.mul(tf(8, 2), o["A"], tz(8, 2)), TypeError,
     "X must be a column-major torch.float64 tensor (e.g. torch.empty(k, n).t())"),
    ("mul-Y-torch-dtype", lambda b, o, s: b.mul(tf(8, 2, torch.float32), o["A"], tf(8, 2)), TypeError,
     "Y must be a column-major torch.float64 tensor (e.g. torch.empty(k, n).t())"),
    ("mul-columns", lambda b, o, s: b.mul(z(8, 3, order="F"), o["A"], z(8, 2, order="F")), ValueError,
     "DimensionMismatch: X and Y have different numbers of columns"),
    # ---- a lockstep solver: the same operand checks under the names B and X, then its own ----------------------------------------
    ("cg-B-length", lambda b, o, s: s["cg"].solve(z(7)), ValueError, "DimensionMismatch: B has shape (7,), expected (8,)"),
    ("cg-B-dtype", lambda b, o, s: s["cg"].solve(z(8, dtype=np.float32)), TypeError, "B must be a contiguous float64 array"),
    ("cg-B-list", lambda b, o, s: s["cg"].solve([0.0] * 8), TypeError, "B must be a numpy array or a torch tensor"),
    ("cg-B-torch-strided", lambda b, o, s: s["cg"].solve(tz(16)[::2]), TypeError, "B must be a contiguous torch.float64 tensor"),
    ("cg-X-length", lambda b, o, s: s["cg"].solve(z(8), z(9)), ValueError, "DimensionMismatch: X has shape (9,), expected (8,)"),
    ("cg-X-matrix-under-B-vector", lambda b, o, s: s["cg"].solve(z(8), z(8, 1, order="F")), ValueError,
     "DimensionMismatch: X has shape (8, 1), expected (8,)"),
    ("cg-B-rows", lambda b, o, s: s["cg"].solve(z(7, 2, order="F")), ValueError, "DimensionMismatch: B must be a 2-D array with 8 rows"),
    ("cg-B-order", lambda b, o, s: s["cg"].solve(z(8, 2)), TypeError, "B must be a column-major (Fortran-order) float64 array"),
    ("cg-B-torch-order", lambda b, o, s: s["cg"].solve(tz(8, 2)), TypeError,
     "B must be a column-major torch.float64 tensor (e.g. torch.empty(k, n).t())"),
    ("cg-X-torch-rows", lambda b, o, s: s["cg"].solve(tf(8, 2), tf(7, 2)), ValueError,
     "DimensionMismatch: X has shape (7, 2), expected (8, k)"),
    ("cg-columns", lambda b, o, s: s["cg"].solve(z(8, 2, order="F"), z(8, 1, order="F")), ValueError,
     "DimensionMismatch: B and X have different numbers of columns"),
    ("cg-too-many-columns", lambda b, o, s: s["cg"].solve(z(8, 3, order="F")), ValueError,
     "B has 3 columns; this solver takes 1 .. 2"),
    ("cg-no-columns", lambda b, o, s: s["cg"].solve(z(8, 0, order="F")), ValueError,
     "B has 0 columns; this solver takes 1 .. 2"),
    ("cg-X0-shape", lambda b, o, s: s["cg"].solve(z(8, 2, order="F"), X0=z(8)), TypeError,
     "X0 must have the shape (8, 2) and the type float64"),
    ("cg-X0-dtype", lambda b, o, s: s["cg"].solve(z(8), X0=z(8, dtype=np.float32)), TypeError,
     "X0 must have the shape (8,) and the type float64"),
    ("cg-X0-torch-dtype", lambda b, o, s: s["cg"].solve(tz(8), X0=tz(8, dtype=torch.complex128)), TypeError,
     "X0 must have the shape (8,) and the type float64"),
    # ---- Gmres: the vector checks under the names b and x, and its own x0 message ------------------------------------------------
    ("gmres-b-length", lambda b, o, s: s["gmres"].solve(z(7)), ValueError, "DimensionMismatch: b has shape (7,), expected (8,)"),
    ("gmres-b-dtype", lambda b, o, s: s["gmres"].solve(z(8, dtype=np.complex128)), TypeError, "b must be a contiguous float64 array"),
    ("gmres-b-strided", lambda b, o, s: s["gmres"].solve(z(16)[::2]), TypeError, "b must be a contiguous float64 array"),
    ("gmres-b-matrix", lambda b, o, s: s["gmres"].solve(z(8, 1, order="F")), ValueError,
     "DimensionMismatch: b has shape (8, 1), expected (8,)"),
    ("gmres-b-torch-length", lambda b, o, s: s["gmres"].solve(tz(7)), ValueError, "DimensionMismatch: b has length (7,), expected 8"),
    ("gmres-x-length", lambda b, o, s: s["gmres"].solve(z(8), z(9)), ValueError, "DimensionMismatch: x has shape (9,), expected (8,)"),
    ("gmres-x-torch-dtype", lambda b, o, s: s["gmres"].solve(tz(8), tz(8, dtype=torch.float32)), TypeError,
     "x must be a contiguous torch.float64 tensor"),
    ("gmres-x0-shape", lambda b, o, s: s["gmres"].solve(z(8), x0=z(7)), TypeError, "x0 must be a vector of 8 entries of float64"),
    ("gmres-x0-dtype", lambda b, o, s: s["gmres"].solve(z(8), x0=z(8, dtype=np.float32)), TypeError,
     "x0 must be a vector of 8 entries of float64"),
    # ---- block lists of the three constructors ------------------------------------------------------------------------------------
    ("bsm-ragged", lambda b, o, s: b.BlockSparseMatrix(_blocks(), I4[:1], I4, (8, 8), device=NODEV), ValueError,
     "blocks, rowindices and colindices must have equal lengths"),
    ("bsm-ragged-cols", lambda b, o, s: b.BlockSparseMatrix(_blocks(), I4, I4 + I4, (8, 8), device=NODEV), ValueError,
     "blocks, rowindices and colindices must have equal lengths"),
    ("bsm-block-shape", lambda b, o, s: b.BlockSparseMatrix(_blocks(), [I4[0], [5, 6, 7]], I4, (8, 8), device=NODEV), ValueError,
     "block shape does not match its index lists"),
    ("bsm-block-3d", lambda b, o, s: b.BlockSparseMatrix([np.zeros((2, 2, 2))], [[1, 2]], [[1, 2]], (8, 8), device=NODEV), ValueError,
     "every block must be a 2-D array"),
    ("bsm-block-type", lambda b, o, s: b.BlockSparseMatrix([np.array([["a"]])], [[1]], [[1]], (8, 8), device=NODEV), TypeError,
     "unsupported block element type <U1"),
    ("sbm-ragged-diagonals", lambda b, o, s: b.SymmetricBlockMatrix(_blocks(), I4[:1], [], [], [], (8, 8), device=NODEV), ValueError,
     "block and index list counts differ"),
    ("sbm-ragged-offdiagonals", lambda b, o, s: b.SymmetricBlockMatrix(_blocks(), I4, [np.ones((4, 4))], [I4[0]], [], (8, 8), device=NODEV),
     ValueError, "block and index list counts differ"),
    ("sbm-diagonal-shape", lambda b, o, s: b.SymmetricBlockMatrix(_blocks(), [I4[0], [5, 6, 7]], [], [], [], (8, 8), device=NODEV), ValueError,
     "diagonal block shape does not match its index list"),
    ("sbm-offdiagonal-shape", lambda b, o, s: b.SymmetricBlockMatrix(_blocks(), I4, [np.ones((4, 3))], [I4[0]], [I4[1]], (8, 8), device=NODEV),
     ValueError, "off-diagonal block shape does not match its index lists"),
    ("sbm-block-3d", lambda b, o, s: b.SymmetricBlockMatrix(_blocks(), I4, [np.ones((4, 4, 1))], [I4[0]], [I4[1]], (8, 8), device=NODEV),
     ValueError, "every block must be a 2-D array"),
    ("vbcrs-ragged-rows", lambda b, o, s: b.VariableBlockCompressedRowStorage(_blocks(), [1], [1, 5], (8, 8), device=NODEV), ValueError,
     "matrices, rowindices and colindices must have equal lengths"),
    ("vbcrs-ragged-cols", lambda b, o, s: b.VariableBlockCompressedRowStorage(_blocks(), [1, 5], [1, 5, 5], (8, 8), device=NODEV), ValueError,
     "matrices, rowindices and colindices must have equal lengths"),
    ("vbcrs-block-3d", lambda b, o, s: b.VariableBlockCompressedRowStorage([np.zeros((2, 2, 2))], [1], [1], (8, 8), device=NODEV), ValueError,
     "every block must be a 2-D array"),
    # ---- the three VBCRS sources refuse an operator without blocks, before anything else ---------------------------------------------
    ("vbcrs-empty-list", lambda b, o, s: b.VariableBlockCompressedRowStorage([], [], [], (8, 8), device=NODEV), IndexError,
     "VariableBlockCompressedRowStorage needs at least one block"),
    ("vbcrs-empty-list-before-storage", lambda b, o, s: b.VariableBlockCompressedRowStorage([], [], [], (8, 8), device=NODEV, storage=np.int32),
     IndexError, "VariableBlockCompressedRowStorage needs at least one block"),
    ("vbcrs-empty-blocksparse", lambda b, o, s: b.VariableBlockCompressedRowStorage(o["E"], device=NODEV, storage=np.int32), IndexError,
     "VariableBlockCompressedRowStorage needs at least one block"),
    ("vbcrs-empty-symmetric-materialised", lambda b, o, s: b.VariableBlockCompressedRowStorage(o["ES"], device=NODEV, materialize=True,
                                                                                                storage=np.int32),
     IndexError, "VariableBlockCompressedRowStorage needs at least one block"),
    # ---- storage= ---------------------------------------------------------------------------------------------------------------------
    ("storage-not-a-dtype", lambda b, o, s: b.BlockSparseMatrix(_blocks(), I4, I4, (8, 8), device=NODEV, storage="nonsense"), TypeError,
     "storage='nonsense' is not a dtype"),
    ("storage-same", lambda b, o, s: b.BlockSparseMatrix(_blocks(), I4, I4, (8, 8), device=NODEV, storage=np.float64), TypeError,
     MIXED % ("float64", "float64")),
    ("storage-of-single", lambda b, o, s: b.SymmetricBlockMatrix(_blocks(np.float32), I4, [], [], [], (8, 8), device=NODEV,
                                                                  storage=np.float32), TypeError, MIXED % ("float32", "float32")),
    ("storage-vbcrs-list", lambda b, o, s: b.VariableBlockCompressedRowStorage(_blocks(), [1, 5], [1, 5], (8, 8), device=NODEV,
                                                                               storage=np.complex64), TypeError, MIXED % ("complex64", "float64")),
    ("storage-vbcrs-from-blocksparse", lambda b, o, s: b.VariableBlockCompressedRowStorage(o["A"], device=NODEV, storage=np.float16),
     TypeError, MIXED % ("float16", "float64")),
    ("storage-vbcrs-from-symmetric", lambda b, o, s: b.VariableBlockCompressedRowStorage(o["S"], device=NODEV, storage=np.float64),
     TypeError, MIXED % ("float64", "float64")),
    ("storage-vbcrs-materialised", lambda b, o, s: b.VariableBlockCompressedRowStorage(o["S"], device=NODEV, materialize=True,
                                                                                       storage=np.float64), TypeError, MIXED % ("float64", "float64")),
    ("storage-devices", lambda b, o, s: b.BlockSparseMatrix(_blocks(), I4, I4, (8, 8), device=NODEV, storage=np.float32, devices=[0]),
     ValueError, "mixed-precision storage is single-device only (devices= is not available)"),
    # ---- invert_blocks keeps its own checks ----------------------------------------------------------------------------------------------
    ("invert-not-square", lambda b, o, s: b.invert_blocks([z(2, 3, order="F")]), ValueError, "a block of shape (2, 3) is not square"),
    ("invert-c-order", lambda b, o, s: b.invert_blocks([z(3, 3)]), TypeError,
     "host blocks must be writeable 2-D Fortran-order numpy arrays of a supported element type"),
    ("invert-read-only", lambda b, o, s: b.invert_blocks([_read_only()]), TypeError,
     "host blocks must be writeable 2-D Fortran-order numpy arrays of a supported element type"),
    ("invert-list-block", lambda b, o, s: b.invert_blocks([[[1.0]]]), TypeError,
     "host blocks must be writeable 2-D Fortran-order numpy arrays of a supported element type"),
    ("invert-integer-block", lambda b, o, s: b.invert_blocks([z(2, 2, dtype=np.int64, order="F")]), TypeError,
     "host blocks must be writeable 2-D Fortran-order numpy arrays of a supported element type"),
    ("invert-two-types", lambda b, o, s: b.invert_blocks([z(2, 2, order="F"), z(2, 2, dtype=np.float32, order="F")]), TypeError,
     "the blocks must share one element type"),
    # ---- a VBCRS that materialised a SymmetricBlockMatrix has no single block list to refresh from ------------------------------------------
    ("materialised-refresh", lambda b, o, s: b.refresh(o["V"]), NotImplementedError, MATERIALISED),
    ("materialised-update-blocks", lambda b, o, s: b.update_blocks(o["V"], []), NotImplementedError, MATERIALISED),
    # ---- update ids (they index the marshalled block list) -----------------------------------------------------------------------------------
    ("refresh-id-range", lambda b, o, s: b.refresh(o["A"], [3]), IndexError, "block id 3 out of range 1..2"),
    ("refresh-id-twice", lambda b, o, s: b.refresh(o["A"], [1, 1]), ValueError, "duplicate block id"),
    # ---- the wrapper check ----------------------------------------------------------------------------------------------------------------------
    ("wrapper-mul", lambda b, o, s: b.mul(z(3), np.eye(3), z(3)), TypeError, "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-mul-transposed", lambda b, o, s: b.mul(z(3), b.transpose(np.eye(3)), z(3)), TypeError,
     "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-submatrices", lambda b, o, s: b.submatrices(np.eye(3), [[1]]), TypeError,
     "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-diag", lambda b, o, s: b.diag(np.eye(3)), TypeError, "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-block-jacobi", lambda b, o, s: b.block_jacobi(np.eye(3), [[1]]), TypeError,
     "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-gmres", lambda b, o, s: b.Gmres(np.eye(3)), TypeError, "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-cg", lambda b, o, s: b.Cg(np.eye(3)), TypeError, "A must be a block matrix or its transpose/adjoint wrapper"),
    ("wrapper-preconditioner", lambda b, o, s: b.BiCgStab(o["A"], np.eye(8)), TypeError,
     "M must be a block matrix or its transpose/adjoint wrapper"),
    ("solver-dtype", lambda b, o, s: b.GmresMulti(o["A"], dtype=np.int32), TypeError, "dtype=int32 is not a supported vector type"),
    # ---- device=True on a handle without a device image ---------------------------------------------------------------------------------------
    ("submatrices-device", lambda b, o, s: b.submatrices(o["A"], [[1, 2]], device=True), ValueError,
     "device=True needs a handle with a device image"),
    ("diag-device", lambda b, o, s: b.diag(o["A"], device=True), ValueError, "device=True needs a handle with a device image"),
    ("submatrices-sets", lambda b, o, s: b.submatrices(o["A"], [[1, 2]], []), ValueError, "one column set per row set"),
]


def _read_only():
    a = np.eye(3, order="F")
    a.flags.writeable = False
    return a


@pytest.mark.parametrize("call,exc,message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refusal_keeps_its_type_and_message(bsm, ops, solvers, call, exc, message):
    with pytest.raises(exc) as ei:
        call(bsm, ops, solvers)
    assert type(ei.value) is exc and str(ei.value) == message


# the package's __all__ before the Python layer was split by concern, name for name
ALL = [
    "SerialScheduler", "DynamicScheduler", "isserial", "AbstractBlockMatrix", "BlockSparseMatrix", "SymmetricBlockMatrix",
    "VariableBlockCompressedRowStorage", "TransposeMap", "AdjointMap", "transpose", "adjoint", "mul", "mul_parts", "MulPlan", "nnz",
    "size", "eltype", "scheduler", "block", "eachblockindex", "rowindices", "colindices", "colors", "transposecolors", "diagonal",
    "offdiagonal", "eachdiagonalindex", "eachoffdiagonalindex", "diagonalindices", "diagonalcolors", "offdiagonalcolors",
    "transposeoffdiagonalcolors", "rowcolvals", "sparse", "ColorInfo", "conflicts", "color", "coloringalgorithm", "Context",
    "partition_rows", "host_register", "host_unregister", "rowcolvals_device", "sparse_device", "update_blocks", "refresh",
    "submatrices", "submatrix", "diag", "invert_blocks", "BlockJacobi", "block_jacobi", "Gmres", "GmresInfo", "gmres", "krylov_orth",
    "krylov_orth_work", "Cg", "CgInfo", "cg", "cocg", "BiCgStab", "bicgstab", "GmresMulti", "synthetic",
]
# entry extraction / export and the preconditioner / solvers have modules of their own; every other name is matrices.py's
ELSEWHERE = {"rowcolvals", "sparse", "rowcolvals_device", "sparse_device", "submatrices", "submatrix", "diag", "invert_blocks",
             "BlockJacobi", "block_jacobi", "Gmres", "GmresInfo", "gmres", "krylov_orth", "krylov_orth_work", "Cg", "CgInfo", "cg",
             "cocg", "BiCgStab", "bicgstab", "GmresMulti", "synthetic"}


def test_public_names_stay_where_callers_find_them(bsm):
    assert sorted(bsm.__all__) == sorted(ALL) and len(set(ALL)) == len(ALL)
    for name in ALL:
        assert hasattr(bsm, name), name
    for name in ALL:
        if name not in ELSEWHERE:
            assert getattr(bsm.matrices, name) is getattr(bsm, name), name
    # what distributed.py and the tests reach through the module beside the public names
    assert bsm.matrices.L is bsm._lib and callable(bsm.matrices.SegmentAdd) and callable(bsm.matrices._options)
