"""The multi-column policy (csrc/bsm_plan.cpp: next_batch, wants_il_arrays) without a device: which kernel takes the next
columns of a product, for every (image dtype, vector dtype) pair, image class, op and column count.

What is expected is written down here from the launchers the plan replaced -- `launch_pair` (the interleaved pass while
enough columns are left), `launch_ladder` (16 / 8 / padded 8 / 4, one stage after the other, each advancing k),
`launch_one` (L of the single columns) and `il_applies` -- as they stood in csrc/bsm_kernels.hip
(today: launch_pair there, the instances in bsm_one.hip / bsm_multi.hip / bsm_il.hip), stage by stage with a
running k (`_model`), and as literal sequences at the documented crossovers.  The library answers through the unexported
hook bsm_debug_plan (plain numbers in, batches out)."""
import ctypes as C
import json
import os
import subprocess
import sys
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, F64, C64, C128, F64_F32, C128_C64 = range(6)
IL, MULTI, ONE = 0, 1, 2
# the eight pairs of launch_mul: same type, mixed storage, complex vectors under a real image
PAIRS = [(F32, F32), (F64, F64), (C64, C64), (C128, C128), (F64_F32, F64), (C128_C64, C128), (F32, C64), (F64, C128)]

Image = namedtuple("Image", "exclusive_fwd has_off colored mean_rows max_rows lane_fill nrows ncols", defaults=(20000, 20000))
CLASSES = {
    "exclusive forward": Image(True, False, False, 64.0, 64, 1.0),
    "forward accumulating, short": Image(False, False, False, 12.0, 28, 0.6),
    "forward accumulating, tall": Image(False, False, False, 64.0, 64, 1.0),
    "symmetric, short": Image(False, True, False, 12.0, 28, 0.6),
    "symmetric, tall": Image(False, True, False, 64.0, 64, 1.0),
    "coloured": Image(False, True, True, 12.0, 28, 0.6),
}
Knobs = namedtuple("Knobs", "multi_il mfma_min il_real_min il_mixed_min mfma_real_min il_xcd", defaults=(1, 3, 5, 0, 0, -1))


def _model(img, dtype, vt, opT, K, arrays, kn=Knobs()):
    """The batches (kind, width, L, kact, row-block instance, XCD run) in the order the replaced launchers issued them."""
    same, cplx = dtype == vt, vt >= C64
    cvec = (dtype, vt) in ((F32, C64), (F64, C128))
    mixed_min = kn.il_mixed_min or (2 if img.has_off else 3)

    def il_applies():
        if K < 2 or kn.multi_il == 0 or img.colored or max(img.nrows, img.ncols) >= 2 ** 30:
            return False
        if cvec:
            return True
        if not same:
            return K >= mixed_min
        if K < (kn.mfma_min if cplx else kn.il_real_min):
            return False
        if not opT and img.exclusive_fwd:
            return False
        return kn.multi_il == 2 or img.mean_rows < 32 or img.has_off

    seq, k = [], 0
    if arrays and il_applies():  # launch_pair
        KK = 8 if cplx else 16
        least = 2 if cvec else mixed_min if not same else kn.mfma_min if cplx else kn.il_real_min
        small = img.max_rows <= 32
        xcd = kn.il_xcd if kn.il_xcd >= 0 else (0 if small else 16)
        while K - k >= least:
            kact = min(KK, K - k)
            seq.append((IL, KK // 2 if kact <= KK // 2 else KK, 0, kact, 2 if small else 4, xcd))
            k += kact
    if same and K > 1:  # launch_ladder
        if not cplx:
            mr_min = kn.mfma_real_min or (15 if img.mean_rows < 32 else 9)
            while K - k >= 16 and mr_min <= 16:
                seq.append((MULTI, 16, 4, 16, 0, 0))
                k += 16
            if mr_min <= K - k < 16:
                seq.append((MULTI, 16, 4, K - k, 0, 0))
                k = K
        while K - k >= 8:
            seq.append((MULTI, 8, 4, 8, 0, 0))
            k += 8
        if K - k >= (kn.mfma_min if cplx else 5):
            seq.append((MULTI, 8, 4, K - k, 0, 0))
            k = K
        if K - k >= 3 or (K - k == 2 and img.lane_fill >= 0.85):
            fwd_only = not opT and (img.exclusive_fwd or not img.has_off)
            seq.append((MULTI, 4, 4 if (not cplx or vt == C128) and not fwd_only else 8, K - k, 0, 0))
            k = K
    while k < K:  # launch_one
        L = 4
        if same:
            L = {F32: 4, F64: 8, C64: 4, C128: 8}[vt]
            if not (img.has_off and not img.exclusive_fwd and (vt != F32 or img.mean_rows < 32)):
                L = 8
        seq.append((ONE, 1, L, 1, 0, 0))
        k += 1
    return seq


_hook = None


def _plan(img, dtype, vt, opT, K, arrays):
    """(the library's batches, its "wants the work arrays")"""
    global _hook
    if _hook is None:
        from bsm_amd import _lib
        _hook = _lib.lib().bsm_debug_plan
        _hook.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_double, C.c_double, C.c_int, C.c_int, C.c_longlong,
                          C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        _hook.restype = C.c_int
    flags = 1 * img.exclusive_fwd + 2 * img.has_off + 4 * img.colored + 8 * opT + 16 * arrays
    out, wants = (C.c_int * (6 * 64))(), C.c_int(-1)
    n = _hook(dtype, vt, img.nrows, img.ncols, img.mean_rows, img.lane_fill, img.max_rows, flags, K, out, 64, C.byref(wants))
    assert 0 <= n <= 64, n
    return [tuple(out[6 * i:6 * i + 6]) for i in range(n)], bool(wants.value)


def _every_case():
    for dtype, vt in PAIRS:
        for name, img in CLASSES.items():
            for opT in (False, True):
                for arrays in (False, True):
                    for K in range(1, 41):
                        yield (dtype, vt, name, opT, arrays, K), img


def test_every_pair_class_op_and_column_count_plans_what_the_launchers_did():
    for case, img in _every_case():
        dtype, vt, _, opT, arrays, K = case
        seq, wants = _plan(img, dtype, vt, opT, K, arrays)
        assert seq == _model(img, dtype, vt, opT, K, arrays), case
        assert sum(b[3] for b in seq) == K and all(1 <= b[3] <= b[1] for b in seq), (case, seq)
        assert arrays or all(b[0] != IL for b in seq), (case, seq)
        assert dtype == vt or all(b[0] != MULTI for b in seq), (case, seq)
        if img.colored or K == 1:
            assert all(b[0] != IL for b in seq), (case, seq)
        # the property mul_k relies on: the arrays are claimed exactly for the products whose plan uses them
        with_arrays = seq if arrays else _plan(img, dtype, vt, opT, K, True)[0]
        assert wants == any(b[0] == IL for b in with_arrays), (case, seq)


def test_images_of_2_to_the_30_rows_or_columns_never_take_the_interleaved_pass():
    for big in (dict(nrows=2 ** 30), dict(ncols=2 ** 30), dict(nrows=2 ** 31 + 5, ncols=2 ** 30)):
        img = CLASSES["symmetric, short"]._replace(**big)
        for dtype, vt in PAIRS:
            for K in range(1, 41):
                seq, wants = _plan(img, dtype, vt, False, K, True)
                assert not wants and all(b[0] != IL for b in seq), (big, dtype, vt, K, seq)
                assert seq == _model(img, dtype, vt, False, K, True)
    # (one below the limit does)
    assert _plan(CLASSES["symmetric, short"]._replace(nrows=2 ** 30 - 1), F64, F64, False, 16, True)[0][0][0] == IL


def _short(seq):
    return [(b[0], b[1], b[3]) for b in seq]


def test_literal_sequences_at_the_documented_crossovers():
    tall, excl = CLASSES["symmetric, tall"], CLASSES["exclusive forward"]
    # fp64 symmetric, tall panels, op N, arrays at hand: the 4-column kernel below BSM_IL_REAL_MIN_COLS = 5
    assert _plan(tall, F64, F64, False, 4, True)[0] == [(MULTI, 4, 4, 4, 0, 0)]
    assert _plan(tall, F64, F64, False, 16, True)[0] == [(IL, 16, 0, 16, 4, 16)]
    assert _plan(tall, F64, F64, False, 20, True)[0] == [(IL, 16, 0, 16, 4, 16), (MULTI, 4, 4, 4, 0, 0)]
    assert _plan(tall, F64, F64, False, 21, True)[0] == [(IL, 16, 0, 16, 4, 16), (IL, 8, 0, 5, 4, 16)]
    # ... without the arrays (a captured graph): the matrix-pipe batch of 16, then the 4-column kernel
    assert _plan(tall, F64, F64, False, 20, False)[0] == [(MULTI, 16, 4, 16, 0, 0), (MULTI, 4, 4, 4, 0, 0)]
    # ComplexF64 symmetric, short panels whose row groups do not fill their lanes (lane_fill < 0.85)
    short = CLASSES["symmetric, short"]
    assert _plan(short, C128, C128, False, 2, True)[0] == [(ONE, 1, 8, 1, 0, 0)] * 2
    assert _plan(short, C128, C128, False, 3, True)[0] == [(IL, 4, 0, 3, 2, 0)]
    assert _plan(short, C128, C128, False, 5, True)[0] == [(IL, 8, 0, 5, 2, 0)]
    # (full lanes: two columns are one padded 4-column pass, L = 4 on the register path)
    assert _plan(tall, C128, C128, False, 2, True)[0] == [(MULTI, 4, 4, 2, 0, 0)]
    # mixed storage, exclusive forward: two columns stay two products, three take the pass
    assert _plan(excl, F64_F32, F64, False, 2, True)[0] == [(ONE, 1, 4, 1, 0, 0)] * 2
    assert _plan(excl, F64_F32, F64, False, 3, True)[0] == [(IL, 8, 0, 3, 4, 16)]
    assert _short(_plan(excl, F64_F32, F64, False, 17, True)[0]) == [(IL, 16, 16), (ONE, 1, 1)]
    assert _plan(excl, F64_F32, F64, False, 8, False)[0] == [(ONE, 1, 4, 1, 0, 0)] * 8
    # ... symmetric: from two columns on
    assert _short(_plan(tall, C128_C64, C128, False, 2, True)[0]) == [(IL, 4, 2)]
    # fp64 exclusive forward (C2-like), op N: never the pass; 16 columns on the matrix pipe from 9 (tall) / 15 (short)
    for arrays in (False, True):
        assert _plan(excl, F64, F64, False, 1, arrays)[0] == [(ONE, 1, 8, 1, 0, 0)]
        assert _plan(excl, F64, F64, False, 8, arrays)[0] == [(MULTI, 8, 4, 8, 0, 0)]
        assert _plan(excl, F64, F64, False, 9, arrays)[0] == [(MULTI, 16, 4, 9, 0, 0)]
        low = excl._replace(mean_rows=31.0)
        assert _plan(low, F64, F64, False, 9, arrays)[0] == [(MULTI, 8, 4, 8, 0, 0), (ONE, 1, 8, 1, 0, 0)]
        assert _plan(low, F64, F64, False, 15, arrays)[0] == [(MULTI, 16, 4, 15, 0, 0)]
    # complex vectors under a real image: the pass from two columns on, exclusive forward images included
    assert _short(_plan(excl, F64, C128, False, 2, True)[0]) == [(IL, 4, 2)]
    assert _short(_plan(excl, F32, C64, False, 13, True)[0]) == [(IL, 8, 8), (IL, 8, 5)]
    assert _plan(excl, F64, C128, False, 3, False)[0] == [(ONE, 1, 4, 1, 0, 0)] * 3
    # fused fp32 products keep 4 loads per lane in flight on SHORT panels only; ComplexF32 on every fused product
    assert _plan(short, F32, F32, False, 1, False)[0] == [(ONE, 1, 4, 1, 0, 0)]
    assert _plan(tall, F32, F32, False, 1, False)[0] == [(ONE, 1, 8, 1, 0, 0)]
    assert _plan(tall, C64, C64, False, 1, False)[0] == [(ONE, 1, 4, 1, 0, 0)]
    assert _plan(excl, C64, C64, False, 1, False)[0] == [(ONE, 1, 8, 1, 0, 0)]


# ---- the knobs: read once per process, so each setting gets a child ------------------------------------------------
def _knob_cases():
    for dtype, vt in PAIRS:
        for name, img in CLASSES.items():
            for opT in (False, True):
                for K in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 33, 40):
                    yield dtype, vt, name, opT, K


def _child(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode())
    cases = list(_knob_cases())
    assert len(got) == len(cases)
    return [(case, [tuple(b) for b in seq]) for case, seq in zip(cases, got)]


@pytest.mark.parametrize("env, kn", [
    ({"BSM_MULTI_IL": "0"}, Knobs(multi_il=0)),
    ({"BSM_MULTI_IL": "2"}, Knobs(multi_il=2)),
    ({"BSM_MULTI_IL": "2", "BSM_IL_XCD": "5"}, Knobs(multi_il=2, il_xcd=5)),
    ({"BSM_IL_XCD": "0"}, Knobs(il_xcd=0)),
    ({"BSM_MFMA_REAL_MIN_COLS": "17"}, Knobs(mfma_real_min=17)),
    ({"BSM_MFMA_MIN_COLS": "5", "BSM_IL_REAL_MIN_COLS": "9"}, Knobs(mfma_min=5, il_real_min=9)),
    ({"BSM_IL_MIXED_MIN_COLS": "1"}, Knobs(il_mixed_min=2)),
    ({"BSM_IL_MIXED_MIN_COLS": "5"}, Knobs(il_mixed_min=5)),
    ({"BSM_IL_MIXED_MIN_COLS": "50"}, Knobs(il_mixed_min=8)),
])
def test_knobs(env, kn):
    seen = set()
    for (dtype, vt, name, opT, K), seq in _child(env):
        img = CLASSES[name]
        assert seq == _model(img, dtype, vt, opT, K, True, kn), (env, dtype, vt, name, opT, K)
        kinds = {(b[0], b[1]) for b in seq}
        seen |= kinds
        if kn.multi_il == 0:  # removes every IL batch of every pair
            assert all(k != IL for k, _ in kinds)
        if kn.multi_il == 2 and name == "forward accumulating, tall" and dtype == vt and K >= (3 if vt >= C64 else 5):
            assert seq[0][0] == IL and _model(img, dtype, vt, opT, K, True)[0][0] != IL  # adds them: not there by default
        if kn.mfma_real_min == 17:  # removes the 16-column multi-RHS kernels
            assert (MULTI, 16) not in kinds
        if kn.il_xcd >= 0:
            assert all(b[5] == kn.il_xcd for b in seq if b[0] == IL)
        if kn.il_mixed_min and dtype >= F64_F32 and not img.colored:  # clamped to 2 .. 8
            assert (seq[0][0] == IL) == (K >= kn.il_mixed_min), (env, name, K, seq)
    assert (MULTI, 8) in seen and (ONE, 1) in seen and ((IL, 16) in seen) == (kn.multi_il != 0)


if __name__ == "__main__":  # the child of test_knobs: the plans of _knob_cases under this process's environment
    print(json.dumps([_plan(CLASSES[name], dtype, vt, opT, K, True)[0] for dtype, vt, name, opT, K in _knob_cases()]))
