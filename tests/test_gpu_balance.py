"""Row groups cut by rows (Analysis::plan_cuts, BSM_WG_CAP) and the balanced dispatch order (BSM_ORDER=2) on the MI355X:
a VBCRS operator of about 3 000 rows whose heavy row segments are cut into unequal chunks computes what the oracle
computes -- every op, both betas, every element type, mixed storage, several right-hand sides, after a refill, through
A[I, J], the COO export and an owned row range that ends inside a cut group -- and an order-only change gives bitwise
the same y.  The knobs are read when a handle is created."""
import numpy as np
import pytest

from _common import NODEV, Cc, N, T, WORK_PANEL, get_image, oracle_mul, rand_vec, relerr
from _gpu import TOL, dev_copy, gpu_mul, gpu_mul_multi, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
HEIGHTS = (8, 9, 16, 17, 31, 32, 33, 63, 64)
HEAVY = {7: 33, 21: 63, 40: 64, 58: 33, 77: 63, 90: 17}  # segment -> height: the segments that carry 6-10 blocks
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


def problem(dtype, seed=0):
    """VBCRS, 100 row segments: heights cycle through HEIGHTS, one or two blocks of 8-40 columns each, the HEAVY ones 6-10
    blocks of 40-72 columns (>= 24 KB in every element type: a workgroup of their own, several times the mean)."""
    rng = np.random.default_rng(seed)
    heights = [HEAVY.get(s, HEIGHTS[s % len(HEIGHTS)]) for s in range(100)]
    n = int(np.sum(heights))
    blocks, rowstart, colstart = [], [], []
    r = 1
    for s, h in enumerate(heights):
        nb = int(rng.integers(6, 11)) if s in HEAVY else int(rng.integers(1, 3))
        c = int(rng.integers(1, 40))
        for _ in range(nb):
            w = int(rng.integers(40, 73)) if s in HEAVY else int(rng.integers(8, 41))
            if c + w - 1 > n:
                break
            blocks.append(np.asfortranarray(rand_vec(rng, h * w, dtype).reshape(h, w)))
            rowstart.append(r)
            colstart.append(c)
            c += w + int(rng.integers(0, 30))
        r += h
    return dict(kind="vbcrs", blocks=blocks, rowstart=np.array(rowstart), colstart=np.array(colstart), size=(n, n))


def heavy_rows(p, s):
    """1-based first row and height of segment s"""
    heights = [HEAVY.get(k, HEIGHTS[k % len(HEIGHTS)]) for k in range(100)]
    return int(np.sum(heights[:s])) + 1, heights[s]


@pytest.fixture
def cut(monkeypatch):
    monkeypatch.setenv("BSM_WG_CAP", "100")


def panel_heights(bsm, p, **kw):
    w = get_image(bsm.synthetic.build(p, device=NODEV, **kw))[3]
    return sorted(set(int(m) for m in w["m"][w["work"] == WORK_PANEL]))


def segment_chunks(bsm, p, s, **kw):
    """(first row, 1-based; rows) of the row groups that produce segment s in an analysis-only twin of the handle"""
    r0, h = heavy_rows(p, s)
    w = get_image(bsm.synthetic.build(p, device=NODEV, **kw))[3]
    lead = w[(w["work"] == WORK_PANEL) & (w["lead"] == 1)]
    got = sorted((int(W["rbase"]) + 1, int(W["m"])) for W in lead if r0 - 1 <= W["rbase"] < r0 - 1 + h)
    assert got[0][0] == r0 and sum(m for _, m in got) == h
    return got


def assert_cut(bsm, p, **kw):
    """every heavy segment of at least 16 rows is cut, and one of them into unequal chunks"""
    chunks = [segment_chunks(bsm, p, s, **kw) for s, h in HEAVY.items() if h >= 33]
    assert all(len(c) > 1 for c in chunks), chunks
    assert any(len(set(m for _, m in c)) > 1 for c in chunks), chunks


def test_the_heavy_segments_are_cut_into_unequal_chunks(bsm, monkeypatch):
    p = problem(np.float64)
    monkeypatch.setenv("BSM_WG_CAP", "0")
    assert set(panel_heights(bsm, p)) == set(HEIGHTS)
    monkeypatch.setenv("BSM_WG_CAP", "100")
    got = set(panel_heights(bsm, p))
    assert got - set(HEIGHTS), "no segment was cut"
    assert got - set(HEIGHTS) - {24, 40, 48, 56}, f"no unequal chunks: {sorted(got)}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_products_with_cuts_against_the_oracle(torch_cuda, bsm, oracle, cut, dtype):
    p = problem(dtype)
    rng = np.random.default_rng(1)
    n = p["size"][0]
    assert_cut(bsm, p)
    A = bsm.synthetic.build(p, transpose_image=True)
    B = bsm.synthetic.build(p)  # op T / C on the forward image (atomics)
    tol = TOL[np.dtype(dtype)]
    for op in (N, T, Cc):
        x, y0 = rand_vec(rng, n, dtype), rand_vec(rng, n, dtype)
        ynan = np.full(n, np.nan, dtype=dtype)
        for H in (A, B):
            got = gpu_mul(torch_cuda, bsm, H, op, x, ynan)  # the strong zero on a NaN-filled y
            assert relerr(got, oracle_mul(oracle, p, op, x, ynan)) < tol, (op, "strong zero")
            got = gpu_mul(torch_cuda, bsm, H, op, x, y0, 0.5, -1.5, False)
            assert relerr(got, oracle_mul(oracle, p, op, x, y0, 0.5, -1.5, False)) < tol, (op, "beta")


def test_float32_storage_under_double_with_cuts(torch_cuda, bsm, oracle, cut):
    p = problem(np.float64)
    rounded = dict(p, blocks=[np.asfortranarray(b.astype(np.float32).astype(np.float64)) for b in p["blocks"]])
    rng = np.random.default_rng(2)
    n = p["size"][0]
    assert_cut(bsm, p, storage=np.float32)
    A = bsm.synthetic.build(p, storage=np.float32, transpose_image=True)
    for op in (N, T, Cc):
        x, y0 = rand_vec(rng, n, np.float64), rand_vec(rng, n, np.float64)
        got = gpu_mul(torch_cuda, bsm, A, op, x, np.full(n, np.nan))
        assert relerr(got, oracle_mul(oracle, rounded, op, x, np.zeros(n))) < TOL[np.dtype(np.float64)]
        assert relerr(got, oracle_mul(oracle, p, op, x, np.zeros(n))) < TOL[np.dtype(np.float32)]
        got = gpu_mul(torch_cuda, bsm, A, op, x, y0, 2.0, 0.25, False)
        assert relerr(got, oracle_mul(oracle, rounded, op, x, y0, 2.0, 0.25, False)) < TOL[np.dtype(np.float64)]


@pytest.mark.parametrize("k", [3, 9])
def test_several_right_hand_sides_with_cuts(torch_cuda, bsm, oracle, cut, k):
    for dtype in (np.float64, np.complex64):
        p = problem(dtype)
        rng = np.random.default_rng(3)
        n = p["size"][0]
        assert_cut(bsm, p)
        A = bsm.synthetic.build(p)
        X = np.asfortranarray(np.stack([rand_vec(rng, n, dtype) for _ in range(k)], axis=1))
        Y0 = np.asfortranarray(np.stack([rand_vec(rng, n, dtype) for _ in range(k)], axis=1))
        for op in (N, T):
            got = gpu_mul_multi(torch_cuda, bsm, A, op, X, Y0, 1.5, 0.5, False, pad=3)
            ref = np.stack([oracle_mul(oracle, p, op, X[:, j].copy(), Y0[:, j].copy(), 1.5, 0.5, False) for j in range(k)], axis=1)
            assert relerr(got.ravel(), ref.ravel()) < TOL[np.dtype(dtype)], (dtype, op)


def test_product_after_update_blocks_with_cuts(torch_cuda, bsm, oracle, cut):
    torch = torch_cuda
    p = problem(np.float64)
    q = dict(p, blocks=[np.asfortranarray(np.random.default_rng(6).standard_normal(b.shape)) for b in p["blocks"]])
    rng = np.random.default_rng(4)
    n = p["size"][0]
    x = rand_vec(rng, n, np.float64)
    for where in ("host", "device"):
        A = bsm.synthetic.build(p, transpose_image=True)
        bsm.update_blocks(A, q["blocks"] if where == "host" else [dev_copy(torch, b) for b in q["blocks"]])
        fresh = bsm.synthetic.build(q, transpose_image=True)
        for op in (N, T):
            got = gpu_mul(torch, bsm, A, op, x, np.full(n, np.nan))
            assert relerr(got, oracle_mul(oracle, q, op, x, np.zeros(n))) < 1e-12, (where, op)
            if op == N:  # the exclusive forward launch is reproducible: bitwise what a fresh handle of the new values gives
                assert np.array_equal(got, gpu_mul(torch, bsm, fresh, op, x, np.full(n, np.nan))), (where, op)
        ids = [3, len(p["blocks"]) // 2, len(p["blocks"])]  # some blocks only, back to the first values
        bsm.update_blocks(A, [p["blocks"][i - 1] for i in ids], ids)
        mixed = dict(q, blocks=[p["blocks"][i] if i + 1 in ids else b for i, b in enumerate(q["blocks"])])
        got = gpu_mul(torch, bsm, A, N, x, np.full(n, np.nan))
        assert relerr(got, oracle_mul(oracle, mixed, N, x, np.zeros(n))) < 1e-12, where


def dense_of(p):
    D = np.zeros(p["size"], dtype=p["blocks"][0].dtype)
    for b, r, c in zip(p["blocks"], p["rowstart"], p["colstart"]):
        D[r - 1:r - 1 + b.shape[0], c - 1:c - 1 + b.shape[1]] += b
    return D


def test_entries_across_a_cut_and_coo_export(torch_cuda, bsm, cut):
    p = problem(np.complex128)
    A = bsm.synthetic.build(p)
    D = dense_of(p)
    for s in (7, 21, 40):
        r0, h = heavy_rows(p, s)
        I = np.arange(r0 - 3, r0 + h + 2)  # 1-based: the whole cut segment and rows of its neighbours
        J = np.arange(1, p["size"][1] + 1, 3)
        assert np.array_equal(bsm.submatrix(A, I, J), D[np.ix_(I - 1, J - 1)]), s
        assert np.array_equal(bsm.submatrix(bsm.transpose(A), J, I), D[np.ix_(I - 1, J - 1)].T), s
    assert np.array_equal(bsm.diag(A), np.diag(D))
    r, c, v = bsm.rowcolvals_device(A, device=False)
    S = np.zeros_like(D)
    np.add.at(S, (np.asarray(r) - 1, np.asarray(c) - 1), np.asarray(v))
    assert len(v) == sum(b.size for b in p["blocks"]) and np.array_equal(S, D)


def test_owned_rows_end_inside_a_cut_group(torch_cuda, bsm, oracle, cut):
    p = problem(np.float64)
    r0, h = heavy_rows(p, 21)  # 63 rows, cut into unequal chunks
    assert h == 63
    n = p["size"][0]
    rng = np.random.default_rng(7)
    x, y0 = rand_vec(rng, n, np.float64), rand_vec(rng, n, np.float64)
    first, second = segment_chunks(bsm, p, 21)[:2]
    assert first[1] != 63, "segment 21 is not cut"
    for hi in (r0 + first[1] // 2, second[0], second[0] + second[1] // 2):  # inside the first chunk, first row of the second, inside the second
        chunks = segment_chunks(bsm, p, 21, own=(5, hi))
        assert len(chunks) > 1 and len(set(m for _, m in chunks)) > 1, "the handle of the owned range must be cut, unequally"
        A = bsm.synthetic.build(p, own=(5, hi))
        got = gpu_mul(torch_cuda, bsm, A, N, x, np.full(n, np.nan))
        assert relerr(got[4:hi], oracle_mul(oracle, p, N, x, np.zeros(n))[4:hi]) < 1e-12, hi
        got = gpu_mul(torch_cuda, bsm, A, N, x, y0, 1.0, 3.0, False)
        assert relerr(got[4:hi], oracle_mul(oracle, p, N, x, y0, 1.0, 3.0, False)[4:hi]) < 1e-12, hi


def test_an_order_only_change_is_bitwise(torch_cuda, bsm, monkeypatch):
    """without cuts BSM_ORDER moves workgroups only: every row's sum is formed by the same waves in the same order"""
    monkeypatch.setenv("BSM_WG_CAP", "0")
    out = {}
    for dtype in (np.float64, np.float32):
        probs = [problem(dtype), bsm.synthetic.config2(n=40_000, nblocks=2000, dtype=dtype)]
        for i, p in enumerate(probs):
            n = p["size"][0]
            x, y0 = rand_vec(np.random.default_rng(8), n, dtype), rand_vec(np.random.default_rng(9), n, dtype)
            for order in ("0", "1", "2"):
                monkeypatch.setenv("BSM_ORDER", order)
                A = bsm.synthetic.build(p)
                out[order] = (gpu_mul(torch_cuda, bsm, A, N, x, np.full(n, np.nan, dtype=dtype)), gpu_mul(torch_cuda, bsm, A, N, x, y0, 0.5, 2.0, False))
            for order in ("0", "1"):
                assert np.array_equal(out[order][0], out["2"][0]) and np.array_equal(out[order][1], out["2"][1]), (dtype, i, order)
