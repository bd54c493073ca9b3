"""CPU suite: the packed image the HIP kernels walk (interpreted by tests/_common.py) against the
oracle on seeded random operators (tests/_fuzz.py) -- the host analysis on layout corner cases."""
import numpy as np
import pytest

from _common import Cc, N, NODEV, T, acc_modes, decode_mixed, get_image, img_bytes, interpret_image, lens, oracle_mul, rand_vec
from _fuzz import GEN, build_fuzz, cast_blocks, fuzz_err, rounded, seed_of


@pytest.fixture(scope="module")
def env():
    import bsm_amd as bsm
    from oracle import load_oracle
    return bsm, load_oracle()


@pytest.mark.parametrize("kind", ["blocksparse", "vbcrs", "symmetric"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_random_operators_interpreted_image_matches_the_oracle(env, kind, dtype):
    bsm, oracle = env
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed_of(kind, dtype) + 1)
    for case in range(8):
        p = GEN[kind](rng, dtype)
        modes = acc_modes(kind)
        acc = modes[case % len(modes)]
        kw = {"accumulate": acc}
        timg = kind != "symmetric" and case % 3 == 0
        if timg:
            kw["transpose_image"] = True
        try:
            A = bsm.synthetic.build(p, device=NODEV, **kw)
        except RuntimeError as e:
            assert acc == "colored" and "repeat" in str(e), (kind, dtype, case, str(e))
            continue
        for op in (N, T, Cc):
            if op == Cc and dtype.kind != "c":
                continue
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, dtype), rand_vec(rng, yl, dtype)
            ref = oracle_mul(oracle, p, op, x, y0, -0.5, 1.25, False)
            got = interpret_image(A, op, x, y0, -0.5, 1.25, False, timage=(timg and op != N))
            assert fuzz_err(got, ref) < 1e-12, (kind, dtype, case, acc, op)


@pytest.mark.parametrize("kind", ["blocksparse", "symmetric"])
def test_random_operators_coarser_wave_records_match_the_oracle(env, kind, monkeypatch):
    """The second wave-record list the multi-RHS kernels walk (bsm_get_image 8), forced onto small random operators
    (2 KB per wave against waves of 256 bytes): same products through the image interpreter."""
    bsm, oracle = env
    monkeypatch.setenv("BSM_WAVE_BYTES", "256")
    monkeypatch.setenv("BSM_MULTI_WAVE_BYTES", "2048")
    dtype = np.dtype(np.float64)
    rng = np.random.default_rng(seed_of(kind, dtype) + 7)
    seen = 0
    for case in range(10):
        p = GEN[kind](rng, dtype)
        A = bsm.synthetic.build(p, device=NODEV, accumulate="atomic")
        if len(get_image(A, multi=True)[3]) == 0:
            continue
        seen += 1
        for op in (N, T):
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, dtype), rand_vec(rng, yl, dtype)
            ref = oracle_mul(oracle, p, op, x, y0, -0.5, 1.25, False)
            got = interpret_image(A, op, x, y0, -0.5, 1.25, False, multi=True)
            assert fuzz_err(got, ref) < 1e-12, (kind, case, op)
    assert seen >= 3


# ---- cross-type pairs and the coloured mode on layout-edge operators ------------------------------------------------
# Coloured cases follow _fuzz.build_fuzz: block-sparse operators are drawn colourable and always build, a symmetric
# operator that repeats a pair of row sets is redrawn up to five times; a test asserts that at least half of its coloured
# cases ran.  (The tests above keep their streams and their `continue`.)
MIXED = [(np.float64, np.float32), (np.complex128, np.complex64)]
KINDS = ["blocksparse", "vbcrs", "symmetric"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T_, S_", MIXED)
def test_mixed_storage_decoded_image_matches_the_oracle_on_rounded_blocks(env, kind, T_, S_):
    """Mixed-storage handles of random operators, every accumulation mode: the packed single-precision image decoded in
    double (decode_mixed: the kernels' arithmetic without their schedule) against the oracle on the rounded blocks"""
    bsm, oracle = env
    T_ = np.dtype(T_)
    rng = np.random.default_rng(seed_of(kind, T_) + 11)
    modes = acc_modes(kind)
    coloured = ran = 0
    for case in range(12):
        acc = modes[case % len(modes)]
        timg = kind != "symmetric" and case % 3 == 0
        kw = {"transpose_image": True} if timg else {}
        p, A = build_fuzz(bsm, rng, kind, T_, acc, device=NODEV, storage=S_, **kw)
        coloured += acc == "colored"
        if A is None:
            continue
        ran += acc == "colored"
        assert A.dtype == T_ and A.storage_dtype == np.dtype(S_)
        q = rounded(p, S_)
        for op in (N, T, Cc):
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, T_), rand_vec(rng, yl, T_)
            ref = oracle_mul(oracle, q, op, x, y0, -0.5, 1.25, False)
            got = decode_mixed(A, op, x, y0, -0.5, 1.25, False, timage=(timg and op != N))
            assert fuzz_err(got, ref) < 1e-12, (kind, T_, case, acc, op)
    assert 2 * ran >= coloured, (kind, T_, ran, coloured)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T_, S_", MIXED)
def test_mixed_values_image_is_that_of_the_blocks_cast_to_the_stored_type(env, kind, T_, S_):
    """what test_mixed_storage_cpu.py::test_mixed_image_equals_rounded_single_image asserts on regular shapes: values,
    rows and columns of a mixed image (and of its transposed ordering) byte for byte those of a single-precision handle"""
    bsm, _ = env
    T_ = np.dtype(T_)
    rng = np.random.default_rng(seed_of(kind, T_) + 12)
    modes = acc_modes(kind)
    coloured = ran = 0
    for case in range(12):
        acc = modes[case % len(modes)]
        timg = kind != "symmetric" and case % 3 == 0
        kw = {"transpose_image": True} if timg else {}
        p, A = build_fuzz(bsm, rng, kind, T_, acc, device=NODEV, storage=S_, **kw)
        coloured += acc == "colored"
        if A is None:
            continue
        ran += acc == "colored"
        with np.errstate(over="ignore"):
            As = bsm.synthetic.build(cast_blocks(p, S_), device=NODEV, accumulate=acc, **kw)
        assert As.dtype == As.storage_dtype == np.dtype(S_)
        for which in (0, 1, 2) + ((16, 17, 18) if timg else ()):
            a = img_bytes(A, which)
            assert len(a) > 0 or which != 0 or A.stats()["stored_entries"] == 0
            assert np.array_equal(a, img_bytes(As, which)), (kind, T_, case, acc, which)
    assert 2 * ran >= coloured, (kind, T_, ran, coloured)


@pytest.mark.parametrize("kind", ["blocksparse", "symmetric"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_coloured_mode_builds_on_colourable_operators_and_matches_the_oracle(env, kind, dtype):
    """Every case coloured.  Block-sparse operators drawn with colourable=True always build (no `continue`); symmetric
    ones after at most five redraws, at least half of them"""
    bsm, oracle = env
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed_of(kind, dtype) + 13)
    ran = 0
    for case in range(12):
        timg = kind != "symmetric" and case % 3 == 0
        kw = {"transpose_image": True} if timg else {}
        p, A = build_fuzz(bsm, rng, kind, dtype, "colored", device=NODEV, **kw)
        if kind == "blocksparse":
            assert A is not None
        if A is None:
            continue
        ran += 1
        for op in (N, T, Cc):
            if op == Cc and dtype.kind != "c":
                continue
            xl, yl = lens(p, op)
            x, y0 = rand_vec(rng, xl, dtype), rand_vec(rng, yl, dtype)
            ref = oracle_mul(oracle, p, op, x, y0, -0.5, 1.25, False)
            got = interpret_image(A, op, x, y0, -0.5, 1.25, False, timage=(timg and op != N))
            assert fuzz_err(got, ref) < 1e-12, (kind, dtype, case, op)
    assert ran == 12 if kind == "blocksparse" else 2 * ran >= 12, (kind, dtype, ran)
