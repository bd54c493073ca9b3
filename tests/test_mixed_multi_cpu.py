"""bsm_value_passes without a GPU: the prototype in include/bsm_rocm.h, the refusals, and the answer of a handle that
has never enqueued a product (analysis-only, BSM_DEVICE_NONE)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _common import NODEV
from _fuzz import cast_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsm_rocm.h")


def test_value_passes_is_declared_with_the_documented_signature():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    m = re.search(r"\bint\s+bsm_value_passes\s*\(([^)]*)\)\s*;", hdr)
    assert m, "int bsm_value_passes(...) is not declared in include/bsm_rocm.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["bsm_matrix_t A", "int64_t *count"]
    from bsm_amd import _lib as L
    assert "bsm_value_passes" in L.EXPORTS and hasattr(L.lib(), "bsm_value_passes")
    fn = L.lib().bsm_value_passes
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(C.c_int64)]


@pytest.mark.parametrize("dt, storage", [(np.float64, None), (np.float64, np.float32), (np.complex128, np.complex64)])
def test_value_passes_refusals_and_a_fresh_analysis_only_handle(bsm, dt, storage):
    from bsm_amd import _lib as L
    fn = L.lib().bsm_value_passes
    n = C.c_int64(-7)
    assert fn(None, C.byref(n)) == -1 and n.value == -7            # BSM_ERR_INVALID: null handle, *count untouched
    p = cast_blocks(bsm.synthetic.config3(nseg=6, bs=8, halfband=1), dt)
    A = bsm.synthetic.build(p, device=NODEV, storage=storage)
    assert fn(A._h.ptr, None) == -1                                 # BSM_ERR_INVALID: null pointer
    assert fn(A._h.ptr, C.byref(n)) == 0 and n.value == 0           # nothing has streamed the image
    assert A.value_passes() == 0
