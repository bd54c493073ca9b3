"""CPU suite: mixed-precision handles (BSM_F64_F32, BSM_C128_C64) -- values stored in single precision under
double-precision vectors.  Analysis-only handles (BSM_DEVICE_NONE): the packed image must be exactly the image of a
pure single-precision handle of the rounded blocks, the bookkeeping that of the pure double-precision handle, the
statistics must count stored bytes for the values and vector bytes for x / y, and the image decoded in fp64 must
reproduce the oracle on the rounded blocks.  Plus the refusals and the mirror's `storage=` checks."""
import ctypes as C

import numpy as np
import pytest

from _common import (Cc, N, NODEV, T, WORK_PANEL, decode_mixed, fixture_problem, get_image, img_bytes, oracle_mul, rand_vec,
                     relerr)
from _ctors import CTORS, ctor_build, ctor_oracle_problem, ctor_problem
from _fuzz import cast_blocks, rounded

OPS = [N, T, Cc]
PAIRS = [(np.float64, np.float32), (np.complex128, np.complex64)]
SIZES = {"blocksparse": dict(n=400, nblocks=40, bs=12), "vbcrs": dict(n=3000, nblocks=160, lo=4, hi=40),
         "vbcrs_from_blocksparse": dict(n=2000, nblocks=120, lo=4, hi=40), "symmetric": dict(nseg=10, bs=20, halfband=2),
         "vbcrs_from_symmetric": dict(nseg=10, bs=20, halfband=2)}


def _bookkeeping_equal(A, B):
    from bsm_amd import _lib as L
    for which in range(7):
        try:
            a = A._bookkeeping(which)
        except L.BsmError:
            with pytest.raises(L.BsmError):
                B._bookkeeping(which)
            continue
        assert np.array_equal(a, B._bookkeeping(which)), f"bookkeeping {which}"


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", CTORS)
def test_mixed_image_equals_rounded_single_image(bsm, oracle, ctor, T_, S_):
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, device=NODEV, storage=S_)
    As = ctor_build(bsm, ctor, cast_blocks(p, S_), device=NODEV)
    At = ctor_build(bsm, ctor, p, device=NODEV)
    assert A.dtype == np.dtype(T_) and A.storage_dtype == np.dtype(S_)
    assert bsm.eltype(A) == np.dtype(T_)
    assert As.storage_dtype == As.dtype == np.dtype(S_)
    # the packed image: byte for byte the single-precision handle's (values, rows, cols)
    for which in (0, 1, 2):
        assert np.array_equal(img_bytes(A, which), img_bytes(As, which)), f"image array {which}"
    # reference bookkeeping: that of the double-precision handle (and of the single one -- it is value-blind)
    _bookkeeping_equal(A, At)
    for attr in ("perm", "rowptr", "colindices", "rowindices"):
        if hasattr(At, attr) and isinstance(getattr(At, attr), np.ndarray):
            assert np.array_equal(getattr(A, attr), getattr(At, attr))
    # statistics: stored bytes for the values, vector bytes for x and y
    st, ss, stt = A.stats(), As.stats(), At.stats()
    assert st["stored_entries"] == stt["stored_entries"] == ss["stored_entries"]
    assert st["nnz"] == stt["nnz"]
    ts, tt = np.dtype(S_).itemsize, np.dtype(T_).itemsize
    nrows, ncols = A.size
    assert st["alg_bytes"] == stt["alg_bytes"] - st["stored_entries"] * (tt - ts)
    assert st["alg_bytes"] == ss["alg_bytes"] + (nrows + ncols) * (tt - ts)
    assert st["device_bytes"] == ss["device_bytes"]  # (no gather workspace: values + metadata only)
    # the image decoded in fp64 against the oracle on the ROUNDED blocks
    orc_p = ctor_oracle_problem(ctor, rounded(p, S_))
    rng = np.random.default_rng(11)
    n = A.size[0]
    x = rand_vec(rng, n, T_)
    y0 = rand_vec(rng, n, T_)
    for op in OPS:
        for alpha, beta, strong in ((1, 0, True), (0.5, 2.0, False)):
            ref = oracle_mul(oracle, orc_p, op, x, y0, alpha, beta, strong)
            got = decode_mixed(A, op, x, y0, alpha, beta, strong)
            assert relerr(got, ref) <= 1e-14, (op, alpha, beta)


@pytest.mark.parametrize("T_, S_", PAIRS)
@pytest.mark.parametrize("ctor", ["blocksparse", "vbcrs"])
def test_mixed_transposed_image(bsm, oracle, ctor, T_, S_):
    p = ctor_problem(bsm, ctor, T_, SIZES)
    A = ctor_build(bsm, ctor, p, device=NODEV, storage=S_, transpose_image=1)
    As = ctor_build(bsm, ctor, cast_blocks(p, S_), device=NODEV, transpose_image=1)
    assert len(img_bytes(A, 16)) > 16  # the handle has a transposed ordering
    for which in (16, 17, 18):
        assert np.array_equal(img_bytes(A, which), img_bytes(As, which)), f"transposed image array {which}"
    orc_p = ctor_oracle_problem(ctor, rounded(p, S_))
    rng = np.random.default_rng(5)
    x = rand_vec(rng, A.size[0], T_)
    y0 = rand_vec(rng, A.size[1], T_)
    for op in (T, Cc):
        ref = oracle_mul(oracle, orc_p, op, x, y0, 0.5, 2.0, False)
        assert relerr(decode_mixed(A, op, x, y0, 0.5, 2.0, False, timage=True), ref) <= 1e-14


@pytest.mark.parametrize("key", ["cuboid", "sphere"])
@pytest.mark.parametrize("ctor", ["symmetric", "vbcrs_from_symmetric"])
def test_mixed_golden_fixtures(bsm, oracle, key, ctor):
    p = fixture_problem(key)  # ComplexF64 BEM near field (the reference's own fixture)
    A = ctor_build(bsm, ctor, p, device=NODEV, storage=np.complex64)
    As = ctor_build(bsm, ctor, cast_blocks(p, np.complex64), device=NODEV)
    for which in (0, 1, 2):
        assert np.array_equal(img_bytes(A, which), img_bytes(As, which))
    orc_p = ctor_oracle_problem(ctor, rounded(p, np.complex64))
    rng = np.random.default_rng(3)
    x = rand_vec(rng, A.size[0], np.complex128)
    y0 = rand_vec(rng, A.size[0], np.complex128)
    for op in OPS:
        ref = oracle_mul(oracle, orc_p, op, x, y0, 1j, 0.5, False)
        assert relerr(decode_mixed(A, op, x, y0, 1j, 0.5, False), ref) <= 1e-14
    # against the ORIGINAL blocks: within single-precision rounding, far from the fp64 result
    ref = oracle_mul(oracle, ctor_oracle_problem(ctor, p), N, x, y0)
    err = relerr(decode_mixed(A, N, x, y0), ref)
    assert 1e-10 < err < 1e-5


def test_mixed_gather_workspace_is_double(bsm):
    p = ctor_problem(bsm, "symmetric", np.float64, SIZES)
    A = ctor_build(bsm, "symmetric", p, device=NODEV, storage=np.float32, accumulate="gather")
    As = ctor_build(bsm, "symmetric", cast_blocks(p, np.float32), device=NODEV, accumulate="gather")
    _, _, cols, waves = get_image(A)
    lead_rows = int(np.sum(waves["m"][(waves["work"] == WORK_PANEL) & (waves["lead"] == 1)]))
    slots = len(cols) + lead_rows + 8
    assert A.stats()["device_bytes"] == As.stats()["device_bytes"] + slots * 4


def test_rounding_is_numpy_astype(bsm):
    """one rounding at pack time, IEEE round-to-nearest-even: subnormals kept, overflow to +-inf, ties to even"""
    f32 = np.finfo(np.float32)
    special = np.array([1e-40, -3e-42, 1e-46, 3.5e38, -1e39, f32.max, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24,
                        np.pi, -np.e, 0.0, -0.0, 2.0 ** -149, 1.5 * 2.0 ** -149], dtype=np.float64)
    blk = np.asfortranarray(np.resize(special, (16, 4)))
    for T_, S_, b in ((np.float64, np.float32, blk), (np.complex128, np.complex64, blk + 1j * blk[::-1])):
        b = np.asfortranarray(b)
        M = bsm.matrices
        A = M.VariableBlockCompressedRowStorage([b], [1], [1], (16, 4), device=NODEV, storage=S_)
        with np.errstate(over="ignore"):
            bs = np.asfortranarray(b.astype(S_))
        As = M.VariableBlockCompressedRowStorage([bs], [1], [1], (16, 4), device=NODEV)
        assert np.array_equal(img_bytes(A, 0), img_bytes(As, 0))
        vals = img_bytes(A, 0).view(S_)
        assert np.isinf(vals.real).sum() > 0 and np.any((vals.real != 0) & (np.abs(vals.real) < f32.tiny))


def test_mixed_refusals(bsm):
    from bsm_amd import _lib as L
    lib = L.lib()
    p = ctor_problem(bsm, "blocksparse", np.float64, SIZES)
    A = ctor_build(bsm, "blocksparse", p, device=NODEV, storage=np.float32)
    # bsm_update_blocks: BSM_ERR_UNSUPPORTED, through the C ABI and the mirror
    ld = np.array([b.shape[0] for b in p["blocks"]], dtype=np.int64)
    ptrs = (C.c_void_p * len(p["blocks"]))(*[b.ctypes.data for b in A.blocks])
    rc = lib.bsm_update_blocks(A._h.ptr, len(p["blocks"]), None, ptrs, ld.ctypes.data_as(C.POINTER(C.c_int64)),
                               L.BSM_MEM_HOST, None)
    assert rc == -2 and b"mixed-precision" in lib.bsm_last_error()
    with pytest.raises(NotImplementedError):
        bsm.update_blocks(A, [p["blocks"][0]], ids=[1])
    with pytest.raises(NotImplementedError):
        bsm.refresh(A)
    # bsm_vec_add_segments takes vector types only
    for code in (L.BSM_F64_F32, L.BSM_C128_C64):
        assert lib.bsm_vec_add_segments(code, None, 0, None, None, None, None) == -1
        assert b"vector type" in lib.bsm_last_error()
    # an unknown code is still unknown
    with pytest.raises(L.BsmError, match="unknown dtype"):
        from bsm_amd.matrices import _options, SerialScheduler
        o = _options(SerialScheduler(), NODEV, "auto")
        h = C.c_void_p()
        blk = np.asfortranarray(np.ones((2, 2)))
        one = np.array([1], dtype=np.int64)
        two = np.array([2], dtype=np.int64)
        I = C.POINTER(C.c_int64)
        L.check(lib.bsm_vbcrs_create(6, 2, 2, 1, (C.c_void_p * 1)(blk.ctypes.data), two.ctypes.data_as(I),
                                     two.ctypes.data_as(I), two.ctypes.data_as(I), one.ctypes.data_as(I),
                                     one.ctypes.data_as(I), C.byref(o), C.byref(h)))
    # multi-device handles: refused before any device is touched (the context is never dereferenced)
    from bsm_amd.matrices import _options, SerialScheduler
    o = _options(SerialScheduler(), NODEV, "auto")
    o.ctx = C.c_void_p(1)
    h = C.c_void_p()
    blk = np.asfortranarray(np.ones((2, 2)))
    one = np.array([1], dtype=np.int64)
    two = np.array([2], dtype=np.int64)
    I = C.POINTER(C.c_int64)
    for code in (L.BSM_F64_F32, L.BSM_C128_C64):
        rc = lib.bsm_vbcrs_create(code, 2, 2, 1, (C.c_void_p * 1)(blk.ctypes.data), two.ctypes.data_as(I),
                                  two.ctypes.data_as(I), two.ctypes.data_as(I), one.ctypes.data_as(I),
                                  one.ctypes.data_as(I), C.byref(o), C.byref(h))
        assert rc == -2 and b"single-device" in lib.bsm_last_error()


def test_mirror_storage_keyword(bsm):
    M = bsm.matrices
    p64 = ctor_problem(bsm, "vbcrs_from_blocksparse", np.float64, SIZES)
    args = (p64["rowindices"], p64["colindices"], p64["size"])
    b32 = [np.asfortranarray(b.astype(np.float32)) for b in p64["blocks"]]
    bc = [np.asfortranarray(b.astype(np.complex128)) for b in p64["blocks"]]
    for blocks, storage in ((p64["blocks"], np.complex64), (p64["blocks"], np.float16), (b32, np.float32),
                            (bc, np.float32), (p64["blocks"], np.float64), (bc, np.complex128), (b32, np.float64),
                            (p64["blocks"], "not a dtype")):
        with pytest.raises(TypeError):
            M.BlockSparseMatrix(blocks, *args, device=NODEV, storage=storage)
    with pytest.raises(ValueError, match="single-device"):
        M.BlockSparseMatrix(p64["blocks"], *args, storage=np.float32, devices=[0, 0])
    A = M.BlockSparseMatrix(p64["blocks"], *args, device=NODEV, storage=np.float32)
    assert A.storage_dtype == np.float32 and A.dtype == np.float64
    V = M.VariableBlockCompressedRowStorage(A, device=NODEV)  # inherits the source's storage
    assert V.storage_dtype == np.float32 and V.dtype == np.float64
    P = M.BlockSparseMatrix(p64["blocks"], *args, device=NODEV)
    assert P.storage_dtype == P.dtype == np.float64
