"""bsm_update_blocks on the MI355X: a refilled handle computes BITWISE what a handle freshly created from the new
values computes (reproducible accumulate modes), for host- and device-resident new blocks, both orderings, several
right-hand sides, multi-device handles; stream order and graph capture as include/bsm_rocm.h promises them."""
import numpy as np
import pytest

from _common import N, T, fixture_problem, oracle_mul, rand_vec, relerr, wrap
from _gpu import dev_copy, torch_cuda  # noqa: F401
from _values import new_values, on_device, padded, raw_update, src_list, with_values

pytestmark = pytest.mark.gpu
C_OP = 2


def products(bsm, torch, A, x, ops=(N, T, C_OP)):
    out = []
    for op in ops:
        M = wrap(bsm, A, op)
        n = A.size[0] if op == N else A.size[1]
        y = torch.zeros(n, dtype=x.dtype, device="cuda")
        bsm.mul(y, M, x)
        out.append(y.cpu().numpy())
    torch.cuda.synchronize()
    return out


def problems(bsm):
    S = bsm.synthetic
    return [("C2", S.config2(n=6000, nblocks=300)), ("C2f32", S.config2(n=5000, nblocks=200, dtype=np.float32)),
            ("C3", S.config3(nseg=24)), ("C3f32", S.config3(nseg=16, dtype=np.float32)),
            ("C4", S.config4_sample(block_rows=(0, 3), block_cols=(1, 2), ngrid=400, bs=32, per_row=6)[0]),
            ("C5", S.config5(n=20_000, lo=16, hi=120, halfband=3)),
            ("fixture", fixture_problem("cuboid"))]


@pytest.mark.parametrize("acc", ["direct", "colored", "gather"])
def test_refill_is_bitwise_a_fresh_handle(torch_cuda, bsm, acc):
    """Bitwise wherever two fresh handles agree bitwise (colored / gather: every op; direct: the exclusive forward
    launch and the transposed image's one-launch T / C -- a product on atomics is compared to rounding instead)."""
    torch = torch_cuda
    rng = np.random.default_rng(1)
    for name, p in problems(bsm):
        x = torch.from_numpy(np.asarray(p["x"]) if "x" in p else rand_vec(rng, p["size"][1], src_list(p)[0].dtype)).cuda()
        vb = new_values(p, rng)
        kw = dict(accumulate=acc) if p["kind"] == "symmetric" else dict(accumulate=acc, transpose_image=True)
        fresh = products(bsm, torch, bsm.synthetic.build(with_values(p, vb), **kw), x)
        again = products(bsm, torch, bsm.synthetic.build(with_values(p, vb), **kw), x)
        tol = 1e-5 if vb[0].dtype in (np.float32, np.complex64) else 1e-12
        for where in ("host", "device"):
            A = bsm.synthetic.build(p if where == "host" else on_device(torch, p), **kw)
            bsm.update_blocks(A, vb if where == "host" else [dev_copy(torch, b) for b in vb])
            got = products(bsm, torch, A, x)
            for k, (g, f, f2) in enumerate(zip(got, fresh, again)):
                if np.array_equal(f, f2):
                    assert np.array_equal(g, f), (name, acc, where, k)
                else:
                    assert relerr(g, f) < tol, (name, acc, where, k)
            assert np.array_equal(got[0], fresh[0]) or not np.array_equal(fresh[0], again[0])


def test_auto_mode_and_transposed_image_against_the_oracle(torch_cuda, bsm, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(2)
    for name, p in problems(bsm):
        vb = new_values(p, rng)
        q = with_values(p, vb)
        dt = vb[0].dtype
        tol = 1e-5 if dt in (np.float32, np.complex64) else 1e-12
        xh = rand_vec(rng, p["size"][1], dt)
        x = torch.from_numpy(xh).cuda()
        tim = p["kind"] != "symmetric"
        A = bsm.synthetic.build(on_device(torch, p), **({"transpose_image": True} if tim else {}))
        bsm.update_blocks(A, [dev_copy(torch, b) for b in vb])
        got = products(bsm, torch, A, x, (N, T))
        for op, g in zip((N, T), got):
            ref = oracle_mul(oracle, q, op, xh, np.zeros(len(g), dtype=dt))
            assert relerr(g, ref) < tol, (name, op)
        if tim:  # the transposed image is bitwise a fresh one too
            Bf = bsm.synthetic.build(q, transpose_image=True, accumulate="direct")
            Ad = bsm.synthetic.build(on_device(torch, p), transpose_image=True, accumulate="direct")
            bsm.update_blocks(Ad, [dev_copy(torch, b) for b in vb])
            assert all(np.array_equal(a, b) for a, b in zip(products(bsm, torch, Ad, x), products(bsm, torch, Bf, x)))


def test_multi_rhs_after_update(torch_cuda, bsm, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    for name, p in problems(bsm)[:3]:
        vb = new_values(p, rng)
        q = with_values(p, vb)
        A = bsm.synthetic.build(p)
        bsm.update_blocks(A, vb)
        n = p["size"][0]
        for K in (8, 16):
            X = np.asfortranarray(rng.standard_normal((n, K)).astype(vb[0].dtype))
            Yd = torch.zeros((K, n), dtype=torch.from_numpy(X).dtype, device="cuda").t()
            bsm.mul(Yd, A, torch.from_numpy(np.ascontiguousarray(X.T)).cuda().t())
            torch.cuda.synchronize()
            ref = np.stack([oracle_mul(oracle, q, N, X[:, k].copy(), np.zeros(n, dtype=X.dtype)) for k in range(K)], axis=1)
            tol = 1e-5 if X.dtype == np.float32 else 1e-12
            assert relerr(Yd.cpu().numpy().ravel(), ref.ravel()) < tol, (name, K)


def test_product_update_product_on_one_stream(torch_cuda, bsm, oracle):
    torch = torch_cuda
    p = bsm.synthetic.config2(n=20_000, nblocks=1500)
    rng = np.random.default_rng(4)
    vb = new_values(p, rng)
    dv = [dev_copy(torch, b) for b in vb]
    A = bsm.synthetic.build(on_device(torch, p))  # device mirror: the update is enqueued on s
    xh = p["x"]
    x = torch.from_numpy(xh).cuda()
    y1 = torch.zeros_like(x)
    y2 = torch.zeros_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bsm.mul(y1, A, x)
        bsm.update_blocks(A, dv, stream=s)
        bsm.mul(y2, A, x)
    torch.cuda.synchronize()
    n = len(xh)
    assert relerr(y1.cpu().numpy(), oracle_mul(oracle, p, N, xh, np.zeros(n))) < 1e-12
    assert relerr(y2.cpu().numpy(), oracle_mul(oracle, with_values(p, vb), N, xh, np.zeros(n))) < 1e-12


def test_update_and_product_in_one_graph(torch_cuda, bsm, oracle):
    torch = torch_cuda
    p = bsm.synthetic.config3(nseg=24)
    rng = np.random.default_rng(5)
    A = bsm.synthetic.build(on_device(torch, p))
    src = A._src()  # the mirror's own device blocks
    n = p["size"][0]
    x = torch.from_numpy(p["x"]).cuda()
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    plan = bsm.MulPlan(y, A, x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bsm.refresh(A, stream=s)  # warm-up: plan upload, table of sources
        plan()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            bsm.refresh(A, stream=s)
            plan()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for _ in range(2):
        vb = new_values(p, rng)
        for d, b in zip(src, vb):
            d.copy_(torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t())  # rewrite the device sources in place
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ref = oracle_mul(oracle, with_values(p, vb), N, p["x"], np.zeros(n))
        assert relerr(y.cpu().numpy(), ref) < 1e-12
    # uncaptured updates from OTHER arrays in between -- device arrays freed afterwards, host blocks through staging
    # windows that are freed too -- do not change what a replay reads: the graph carries its own table
    other = new_values(p, rng)
    tmp = [dev_copy(torch, b) for b in other]
    raw_update(A, range(1, len(tmp) + 1), tmp, [b.shape[0] for b in other], 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del tmp
    raw_update(A, range(1, len(other) + 1), other, [b.shape[0] for b in other], 0)
    vb = new_values(p, rng)
    for d, b in zip(src, vb):
        d.copy_(torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t())
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert relerr(y.cpu().numpy(), oracle_mul(oracle, with_values(p, vb), N, p["x"], np.zeros(n))) < 1e-12


def subset_round(torch, rng, p, A, cur, where, stream):
    """updates a random third of the blocks of A (random order, ld > m) and returns the new constructor-order values"""
    nb = len(cur)
    ids = rng.permutation(nb)[: max(1, nb // 3)] + 1
    fresh = new_values(p, rng)
    arrs, lds = [], []
    for i in ids:
        a, ld = padded(torch, fresh[i - 1], 3, where == "device")
        arrs.append(a)
        lds.append(ld)
    raw_update(A, ids, arrs, lds, 1 if where == "device" else 0, stream)
    out = list(cur)
    for i in ids:
        out[i - 1] = fresh[i - 1]
    return out, arrs


@pytest.mark.parametrize("acc", ["colored", "direct"])
def test_subset_updates_are_bitwise_a_fresh_handle(torch_cuda, bsm, acc):
    """two subset updates in a row (the second rewrites table and item list), random ids in random order, ld > m,
    the transposed image refilled through its own item list, host and device blocks"""
    torch = torch_cuda
    rng = np.random.default_rng(11)
    for name, p in [problems(bsm)[k] for k in (0, 1, 2, 5, 6)]:
        x = torch.from_numpy(np.asarray(p["x"]) if "x" in p else rand_vec(rng, p["size"][1], src_list(p)[0].dtype)).cuda()
        kw = dict(accumulate=acc) if p["kind"] == "symmetric" else dict(accumulate=acc, transpose_image=True)
        tol = 1e-5 if src_list(p)[0].dtype in (np.float32, np.complex64) else 1e-12
        for where in ("host", "device"):
            A = bsm.synthetic.build(p if where == "host" else on_device(torch, p), **kw)
            st = torch.cuda.current_stream().cuda_stream
            cur, keep1 = subset_round(torch, rng, p, A, src_list(p), where, st)
            cur, keep2 = subset_round(torch, rng, p, A, cur, where, st)
            got = products(bsm, torch, A, x)
            fresh = products(bsm, torch, bsm.synthetic.build(with_values(p, cur), **kw), x)
            again = products(bsm, torch, bsm.synthetic.build(with_values(p, cur), **kw), x)
            for k, (g, f, f2) in enumerate(zip(got, fresh, again)):
                if np.array_equal(f, f2):
                    assert np.array_equal(g, f), (name, acc, where, k)
                else:
                    assert relerr(g, f) < tol, (name, acc, where, k)


def test_subset_updates_of_a_multi_device_handle(torch_cuda, bsm, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(12)
    for name, p in [problems(bsm)[k] for k in (0, 2, 5)]:
        for where in ("host", "device"):
            A = bsm.synthetic.build(p if where == "host" else on_device(torch, p), devices=[0, 0, 0])
            cur, keep1 = subset_round(torch, rng, p, A, src_list(p), where, torch.cuda.current_stream().cuda_stream)
            cur, keep2 = subset_round(torch, rng, p, A, cur, where, torch.cuda.current_stream().cuda_stream)
            q = with_values(p, cur)
            dt = cur[0].dtype
            tol = 1e-5 if dt == np.float32 else 1e-12
            xh = rand_vec(rng, p["size"][1], dt)
            y = torch.zeros(p["size"][0], dtype=torch.from_numpy(xh).dtype, device="cuda")
            bsm.mul(y, A, torch.from_numpy(xh).cuda())
            torch.cuda.synchronize()
            assert relerr(y.cpu().numpy(), oracle_mul(oracle, q, N, xh, np.zeros(p["size"][0], dtype=dt))) < tol, (name, where)


def test_host_update_larger_than_a_staging_window(torch_cuda, bsm):
    """108 MB of host blocks (two 64 MB staging windows), all of them in a random order (the item-list path) and then
    a random half, checked bitwise against a fresh handle, both images"""
    torch = torch_cuda
    rng = np.random.default_rng(13)
    p = bsm.synthetic.config2(n=200_000, nblocks=10_000)
    kw = dict(accumulate="colored", transpose_image=True)
    A = bsm.synthetic.build(p, **kw)
    nb = len(p["blocks"])
    assert sum(b.nbytes for b in p["blocks"]) > 64 << 20
    cur = new_values(p, rng)
    ids = rng.permutation(nb) + 1
    raw_update(A, ids, [cur[i - 1] for i in ids], [cur[i - 1].shape[0] for i in ids], 0)
    cur, keep = subset_round(torch, rng, p, A, cur, "host", None)
    x = torch.from_numpy(p["x"]).cuda()
    got = products(bsm, torch, A, x)
    fresh = products(bsm, torch, bsm.synthetic.build(with_values(p, cur), **kw), x)
    for k, (g, f) in enumerate(zip(got, fresh)):
        assert np.array_equal(g, f), k


def test_same_arrays_on_a_second_stream(torch_cuda, bsm, oracle):
    """an update that reuses the previous update's table on ANOTHER stream is ordered behind that update"""
    torch = torch_cuda
    p = bsm.synthetic.config2(n=20_000, nblocks=1500)
    rng = np.random.default_rng(14)
    A = bsm.synthetic.build(on_device(torch, p), accumulate="colored")
    src = A._src()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    bsm.refresh(A, stream=s1)
    vb = new_values(p, rng)
    with torch.cuda.stream(s2):
        for d, b in zip(src, vb):
            d.copy_(torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t())
        bsm.refresh(A, stream=s2)
        x = torch.from_numpy(p["x"]).cuda()
        y = torch.zeros_like(x)
        bsm.mul(y, A, x)
    torch.cuda.synchronize()
    n = len(p["x"])
    assert relerr(y.cpu().numpy(), oracle_mul(oracle, with_values(p, vb), N, p["x"], np.zeros(n))) < 1e-12


def test_multi_device_handle(torch_cuda, bsm, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    for name, p in problems(bsm)[:3] + problems(bsm)[5:6]:
        for where in ("host", "device"):
            A = bsm.synthetic.build(p if where == "host" else on_device(torch, p), devices=[0, 0, 0])
            vb = new_values(p, rng)
            q = with_values(p, vb)
            bsm.update_blocks(A, vb if where == "host" else [dev_copy(torch, b) for b in vb])
            dt = vb[0].dtype
            tol = 1e-5 if dt == np.float32 else 1e-12
            xh = rand_vec(rng, p["size"][1], dt)
            y = torch.zeros(p["size"][0], dtype=torch.from_numpy(xh).dtype, device="cuda")
            bsm.mul(y, A, torch.from_numpy(xh).cuda())
            torch.cuda.synchronize()
            ref = oracle_mul(oracle, q, N, xh, np.zeros(p["size"][0], dtype=dt))
            assert relerr(y.cpu().numpy(), ref) < tol, (name, where)
            parts = A.parts()
            xp = [torch.from_numpy(xh[pp["cols"][0] - 1:pp["cols"][1]].copy()).cuda() for pp in parts]
            yp = [torch.zeros(pp["own"][1] - pp["own"][0] + 1, dtype=y.dtype, device="cuda") for pp in parts]
            bsm.mul_parts(yp, A, xp)
            torch.cuda.synchronize()
            assert relerr(np.concatenate([t.cpu().numpy() for t in yp]), ref) < tol, (name, where, "parts")


def test_mirror_edit_then_refresh(torch_cuda, bsm, oracle):
    torch = torch_cuda
    rng = np.random.default_rng(7)
    for p in (bsm.synthetic.config2(n=6000, nblocks=300), bsm.synthetic.config3(nseg=24)):
        A = bsm.synthetic.build(p, accumulate="colored")  # bitwise reproducible run to run
        xh = p["x"]
        n = len(xh)
        x = torch.from_numpy(xh).cuda()
        y = torch.zeros_like(x)
        bsm.mul(y, A, x)
        torch.cuda.synchronize()
        y0 = y.cpu().numpy()
        src = A._src()
        i = int(rng.integers(len(src)))
        src[i][...] = rng.standard_normal(src[i].shape)  # in place, like block(A, i) .= ...
        bsm.mul(y, A, x)
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy(), y0)  # the image still holds the old values
        bsm.refresh(A)
        bsm.mul(y, A, x)
        torch.cuda.synchronize()
        q = with_values(p, [np.asfortranarray(b) for b in A._src()])
        assert relerr(y.cpu().numpy(), oracle_mul(oracle, q, N, xh, np.zeros(n))) < 1e-12
