"""CPU suite: complex vectors under a real handle (bsm_mul_cvec / bsm_mul_multi_cvec).  What needs no device: the
symbols, the return codes of both entries on analysis-only handles (refusals come before the device check), and the
TypeErrors of the Python mirror for the pairs nobody supports."""
import ctypes as C

import numpy as np
import pytest

from _common import NODEV, Cc, N, T

OK, INVALID, UNSUPPORTED, DEVICE = 0, -1, -2, -3


def _vbcrs(bsm, dt, **kw):
    p = bsm.synthetic.config2(n=600, nblocks=40, lo=4, hi=24)
    blocks = [np.asfortranarray(b.astype(dt)) for b in p["blocks"]]
    if np.dtype(dt).kind == "c":
        blocks = [np.asfortranarray(b + 0.5j * b) for b in blocks]
    kw.setdefault("device", NODEV)
    return bsm.matrices.VariableBlockCompressedRowStorage(blocks, p["rowstart"], p["colstart"], p["size"], **kw)


def _calls(A, op=N, memspace=0, x=True, y=True, nrhs=2):
    """return codes of bsm_mul_cvec and bsm_mul_multi_cvec on handle A (vectors of the handle's length)"""
    from bsm_amd import _lib as L
    n = max(A.size)
    buf = np.zeros(2 * n * max(nrhs, 1), dtype=np.complex128)
    xp = buf.ctypes.data if x else None
    yp = np.zeros_like(buf).ctypes.data if y else None
    h = A._h.ptr if A is not None else None
    one = C.c_int64(max(n, 1))
    rc1 = L.lib().bsm_mul_cvec(h, op, xp, yp, None, None, 1, memspace, None)
    rc2 = L.lib().bsm_mul_multi_cvec(h, op, nrhs, xp, one, yp, one, None, None, 1, memspace, None)
    return rc1, rc2


def test_cvec_symbols_exported():
    from bsm_amd import _lib as L
    lib = L.lib()
    for name in ("bsm_mul_cvec", "bsm_mul_multi_cvec"):
        assert hasattr(lib, name) and name in L.EXPORTS


@pytest.mark.parametrize("dt", [np.complex128, np.complex64])
def test_cvec_refuses_complex_handle(bsm, dt):
    from bsm_amd import _lib as L
    A = _vbcrs(bsm, dt)
    assert _calls(A) == (INVALID, INVALID)
    assert b"bsm_mul" in L.lib().bsm_last_error()


@pytest.mark.parametrize("dt, s", [(np.float64, np.float32), (np.complex128, np.complex64)])
def test_cvec_refuses_mixed_handle(bsm, dt, s):
    A = _vbcrs(bsm, dt, storage=s)
    assert _calls(A) == (UNSUPPORTED, UNSUPPORTED)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_cvec_argument_checks_and_analysis_only(bsm, dt):
    A = _vbcrs(bsm, dt)
    from bsm_amd import _lib as L
    assert L.lib().bsm_mul_cvec(None, N, None, None, None, None, 1, 0, None) == INVALID  # null handle
    assert _calls(A, x=False) == (INVALID, INVALID)
    assert _calls(A, y=False) == (INVALID, INVALID)
    assert _calls(A, op=3) == (INVALID, INVALID)
    assert _calls(A, op=-1) == (INVALID, INVALID)
    assert _calls(A, memspace=2) == (INVALID, INVALID)
    assert _calls(A, nrhs=-1)[1] == INVALID
    assert _calls(A, nrhs=0)[1] == OK  # nothing to do
    for op in (N, T, Cc):  # a real analysis-only handle passes every check but the device one
        for ms in (0, 1):
            assert _calls(A, op=op, memspace=ms) == (DEVICE, DEVICE)


# ---- the Python mirror's refusals ------------------------------------------------------------------------------------
def test_mirror_refuses_unsupported_pairs(bsm):
    A64 = _vbcrs(bsm, np.float64)
    A32 = _vbcrs(bsm, np.float32)
    n = A64.size[0]
    c128, c64, f64 = (np.zeros(n, dtype=t) for t in (np.complex128, np.complex64, np.float64))
    M = bsm.matrices
    # complex alpha / beta with real vectors (unchanged)
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(f64.copy(), A64, f64.copy(), 1 + 1j)
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(f64.copy(), A64, f64.copy(), 1, 2j)
    # precision mismatch
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(c128.copy(), A32, c128.copy())
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(c64.copy(), A64, c64.copy())
    with pytest.raises(TypeError, match="supported pairs"):
        A32 @ c128
    # complex x with real y, and the other way round
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(f64.copy(), A64, c128.copy())
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(c128.copy(), A64, f64.copy())
    # several right-hand sides likewise
    X = np.zeros((n, 3), dtype=np.complex128, order="F")
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(np.zeros((n, 3), order="F"), A64, X)
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(np.zeros((n, 3), dtype=np.complex128, order="F"), A32, X)
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(np.zeros((n, 3), order="F"), A64, np.zeros((n, 3), order="F"), 1j)
    # the transpose / adjoint wrappers
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(c128.copy(), M.transpose(A32), c128.copy())
    with pytest.raises(TypeError, match="supported pairs"):
        bsm.mul(f64.copy(), M.adjoint(A64), c128.copy())


def test_mirror_refuses_mixed_storage_with_complex_vectors(bsm):
    A = _vbcrs(bsm, np.float64, storage=np.float32)
    n = A.size[0]
    with pytest.raises(TypeError, match="mixed-storage"):
        bsm.mul(np.zeros(n, np.complex128), A, np.zeros(n, np.complex128))
    with pytest.raises(TypeError, match="mixed-storage"):
        A @ np.zeros(n, np.complex128)


def test_mirror_takes_the_supported_pairs_to_the_c_entry(bsm):
    """the supported pairs pass the mirror's checks and reach bsm_mul_cvec / bsm_mul_multi_cvec, which answer
    BSM_ERR_DEVICE for an analysis-only handle (raised as RuntimeError by the mirror, not TypeError)"""
    for dt, ct in ((np.float64, np.complex128), (np.float32, np.complex64)):
        A = _vbcrs(bsm, dt)
        n = A.size[0]
        for call in (lambda: bsm.mul(np.zeros(n, ct), A, np.ones(n, ct), 1 - 1j, 0.5j),
                     lambda: A @ np.ones(n, ct),
                     lambda: bsm.mul(np.zeros(n, ct), bsm.matrices.adjoint(A), np.ones(n, ct)),
                     lambda: bsm.mul(np.zeros((n, 3), ct, order="F"), A, np.ones((n, 3), ct, order="F"))):
            with pytest.raises(Exception) as ei:
                call()
            assert not isinstance(ei.value, TypeError)
            assert "device image" in str(ei.value)
