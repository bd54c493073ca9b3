"""GPU suite: the kernels that put VALUES into a handle's packed image or read them out again -- pack_kernel /
pack_convert_kernel (device-resident blocks at construction), refill_kernel (bsm_update_blocks) and export_coo_kernel
(bsm_rowcolvals) -- on the layout-edge operators of tests/_fuzz.py: odd widths that share a 16-byte unit, many tiny
chunks in one wave item, chunk heights that are no power of two, scattered placement of blocks taller than 64 rows, more
than 64 off-diagonal columns in a piece, empty blocks, ld > m on device sources.

The reference is _fuzz.coo_triples: the entries of an operator straight from its numpy blocks.  Every comparison of
triples is exact (_fuzz.canonical: sorted by row, column and the value's bit pattern); test_fuzz_values_cpu.py holds the
host packer, the host replay of the refill plan and the host mirror's rowcolvals to the same reference on the same
operators, and asserts that they reach every layout edge.  A refilled handle starts from NaN blocks, so a slot the
refill misses shows up in the export."""
import functools

import numpy as np
import pytest

from _common import NODEV, WORK_SCALE, Cc, N, T, _image_exclusive, get_image, rand_vec, relerr, wrap
from _fuzz import canonical, coo_triples, edge_features, rounded
from _gpu import TOL, dev_copy, torch_cuda  # noqa: F401
from _values import (MEM_DEVICE, MEM_HOST, NOPS, assert_coverage, explain, nan_blocks, new_values, on_device, options, padded,
                     raw_update, seeded, src_list, subset_of, value_operators, value_seed, with_values)

pytestmark = pytest.mark.gpu
KINDS = ["blocksparse", "vbcrs", "symmetric"]
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
DOUBLES = [(np.float64, np.float32), (np.complex128, np.complex64)]
name_of = lambda d: np.dtype(d).name  # noqa: E731


@functools.lru_cache(maxsize=None)
def operators(kind, dtype):
    """the operators of a (kind, element type) and the canonical triples of each, computed once for every leg"""
    ops = value_operators(kind, dtype)
    assert_coverage(kind, dtype, ops)  # the same operators as the CPU test: its coverage condition carries over
    return ops, [canonical(*coo_triples(p)) for p in ops]


def busiest(ops):
    """the operator with the most blocks: the one that takes the legs only one operator per (kind, type) runs"""
    return max(range(len(ops)), key=lambda k: len(src_list(ops[k])))


def export(bsm, A):
    r, c, v = bsm.rowcolvals_device(A, device=False)
    assert len(r) == len(c) == len(v) == bsm.nnz(A)
    return r, c, v


def check_export(bsm, A, p, want, seed, case, what, same_as=None):
    """the device export of A is the set of triples `want`.  same_as: the raw export of a handle of the same structure
    that passed already -- the order of the export is fixed by the structure, so equal arrays need no second sort."""
    raw = export(bsm, A)
    assert len(raw[0]) == len(want), (seed, case, what, len(raw[0]), len(want))
    if same_as is None or not all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(raw, same_as)):
        got = canonical(*raw)
        assert np.array_equal(got, want), what + ": " + explain(p, seed, case, got, want)
    return raw


def device_blocks(torch, p, pad_every_second=True):
    """p with its blocks in HBM, every second one inside an array with ld = m + 3 whose pad rows hold NaN"""
    out = []
    for k, b in enumerate(src_list(p)):
        if pad_every_second and k % 2 == 1:
            out.append(padded(torch, b, 3, True)[0][:b.shape[0]])
        else:
            out.append(dev_copy(torch, b))
    return with_values(p, out)


def valstat(leg, kind, dtype, nops, ntriples):
    print(f"VALSTAT {leg} {kind} {name_of(dtype)} operators {nops} triples {ntriples}")


# ---- 1. export_coo_kernel on images the host packer wrote -----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_export_of_a_host_packed_image(torch_cuda, bsm, kind, dtype):
    ops, refs = operators(kind, dtype)
    seed = value_seed(kind, dtype)
    total = views = 0
    for case, (p, want) in enumerate(zip(ops, refs)):
        A = bsm.synthetic.build(p, **options(kind, case))
        check_export(bsm, A, p, want, seed, case, "host arrays")
        r, c, v = bsm.rowcolvals_device(A, device=True)  # triples written into device arrays
        got = canonical(r.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy())
        assert np.array_equal(got, want), "device arrays: " + explain(p, seed, case, got, want)
        total += len(want)
        if kind == "symmetric" and "scattered" not in edge_features(p):
            # the VBCRS view of a symmetric operator (the symmetric image under VBCRS bookkeeping) places every block
            # at the FIRST index of its lists: the same matrix where the lists are contiguous
            V = bsm.VariableBlockCompressedRowStorage(A)
            check_export(bsm, V, p, want, seed, case, "VBCRS view")
            views += 1
    if kind == "symmetric":
        assert views >= 2, (seed, views)
    valstat("export", kind, dtype, NOPS, total)


# ---- 2. pack_kernel: blocks device-resident at construction ------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_device_pack(torch_cuda, bsm, kind, dtype):
    ops, refs = operators(kind, dtype)
    seed = value_seed(kind, dtype)
    for case, (p, want) in enumerate(zip(ops, refs)):
        kw = options(kind, case)
        Ad = bsm.synthetic.build(device_blocks(torch_cuda, p), **kw)
        check_export(bsm, Ad, p, want, seed, case, "device pack")
        assert Ad.stats() == bsm.synthetic.build(p, **kw).stats(), (seed, case)
    valstat("pack", kind, dtype, NOPS, sum(len(w) for w in refs))


def test_regression_empty_device_block_is_accepted(torch_cuda, bsm):
    """blocksparse float32, case 0, block 6 (0 x 16): the CUDA copy of an empty block has stride 0 along its columns, and
    the mirror's column-major check refused it (TypeError) although a block without entries has no layout"""
    ops, refs = operators("blocksparse", np.float32)
    p, want = ops[0], refs[0]
    assert src_list(p)[5].shape == (0, 16)
    q = on_device(torch_cuda, p)
    assert q["blocks"][5].stride(1) == 0
    A = bsm.synthetic.build(q, **options("blocksparse", 0))
    check_export(bsm, A, p, want, value_seed("blocksparse", np.float32), 0, "device blocks, one of them empty")
    bsm.refresh(A)  # the same check in front of an update from the mirror's device blocks
    check_export(bsm, A, p, want, value_seed("blocksparse", np.float32), 0, "after refresh")


# ---- 3. pack_convert_kernel: mixed storage ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T_, S_", DOUBLES, ids=name_of)
def test_converting_pack(torch_cuda, bsm, kind, T_, S_):
    """mixed storage: the export of a handle packed from host blocks and of one packed from device blocks is, bit for bit,
    astype(S).astype(T) of the blocks -- among them values that truncation would round otherwise, values subnormal in
    single precision and values beyond its range (_values.SPECIAL)"""
    ops, _ = operators(kind, T_)
    seed = value_seed(kind, T_)
    total = 0
    for case, p in enumerate(ops):
        q = seeded(p)
        with np.errstate(over="ignore"):
            want = canonical(*coo_triples(rounded(q, S_)))
        kw = dict(options(kind, case), storage=S_)
        Ah = bsm.synthetic.build(q, **kw)
        raw_h = check_export(bsm, Ah, q, want, seed, case, "host blocks")
        Ad = bsm.synthetic.build(device_blocks(torch_cuda, q), **kw)
        raw_d = check_export(bsm, Ad, q, want, seed, case, "device blocks", same_as=raw_h)
        assert raw_h[2].dtype == np.dtype(T_)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(raw_h, raw_d)), (seed, case)
        total += len(want)
    valstat("convert", kind, T_, NOPS, total)


# ---- 4. refill_kernel, forward image ----------------------------------------------------------------------------------
def sources(torch, blocks, where, pad):
    """blocks as arrays of memory space `where` (pad: inside arrays with ld = m + pad, NaN in the pad rows) -> arrays, lds"""
    arrs, lds = [], []
    for b in blocks:
        if pad:
            a, ld = padded(torch, b, pad, where == "device")
        else:
            a, ld = (dev_copy(torch, b) if where == "device" else b), max(b.shape[0], 1)
        arrs.append(a)
        lds.append(ld)
    return arrs, lds


def update(torch, A, ids, blocks, where, pad=0):
    arrs, lds = sources(torch, blocks, where, pad)
    raw_update(A, ids, arrs, lds, MEM_DEVICE if where == "device" else MEM_HOST, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()  # (the device sources are let go below)


def rounds(rng, p):
    """the values a refilled handle goes through: all of p's, then two subset updates -> [(ids, blocks, pad, problem)]"""
    cur = src_list(p)
    out = [(range(1, len(cur) + 1), cur, 0, p)]
    for _ in range(2):
        ids, blocks, cur = subset_of(rng, p, cur)
        out.append((ids, blocks, 3, with_values(p, cur)))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_refill_of_the_forward_image(torch_cuda, bsm, kind, dtype):
    """a handle built from NaN blocks, refilled with every block and then twice with a random third of them (random order,
    ld = m + 3, NaN in the pad rows) exports the current values after each update -- host- and device-block updates on
    handles created from host and from device blocks"""
    torch = torch_cuda
    ops, refs = operators(kind, dtype)
    seed = value_seed(kind, dtype)
    rng = np.random.default_rng(seed + 4)
    total = 0
    for case, (p, want0) in enumerate(zip(ops, refs)):
        plan = rounds(rng, p)
        wants = [want0] + [canonical(*coo_triples(q)) for _, _, _, q in plan[1:]]
        hollow = nan_blocks(p)
        first = [None] * len(plan)
        for built in ("host", "device"):
            for where in ("host", "device"):
                A = bsm.synthetic.build(hollow if built == "host" else on_device(torch, hollow), **options(kind, case))
                for k, ((ids, blocks, pad, q), want) in enumerate(zip(plan, wants)):
                    update(torch, A, ids, blocks, where, pad)
                    raw = check_export(bsm, A, q, want, seed, case, f"built from {built} blocks, {where} update {k}",
                                       same_as=first[k])
                    first[k] = raw if first[k] is None else first[k]
        total += sum(len(w) for w in wants)
    valstat("refill", kind, dtype, NOPS, total)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_captured_refill(torch_cuda, bsm, kind, dtype):
    """refresh captured into a graph (after one uncaptured refresh): the device sources rewritten in place, one replay,
    and the export holds the new values"""
    torch = torch_cuda
    ops, _ = operators(kind, dtype)
    seed = value_seed(kind, dtype)
    case = busiest(ops)
    p = ops[case]
    rng = np.random.default_rng(seed + 5)
    A = bsm.synthetic.build(on_device(torch, nan_blocks(p)), **options(kind, case))
    src = A._src()  # the mirror's own device blocks
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bsm.refresh(A, stream=s)  # uncaptured: plan upload, table of sources
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            bsm.refresh(A, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    vb = new_values(p, rng)
    for d, b in zip(src, vb):
        d.copy_(dev_copy(torch, b))  # rewrite the device sources in place
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    q = with_values(p, vb)
    want = canonical(*coo_triples(q))
    check_export(bsm, A, q, want, seed, case, "captured refresh")
    valstat("captured", kind, dtype, 1, len(want))


# ---- 5. refill_kernel and pack_kernel, transposed image ---------------------------------------------------------------
def one_column_products(bsm, torch, A, xs):
    out = []
    for op, x in zip((N, T, Cc), xs):
        M = wrap(bsm, A, op)
        y = torch.zeros(A.size[0] if op == N else A.size[1], dtype=x.dtype, device="cuda")
        bsm.mul(y, M, x)
        out.append(y.cpu().numpy())
    return out


def exclusive_products(bsm, p, kw):
    """which of the products N, T, C of a transpose_image handle of p are ONE launch of plain stores (bitwise reproducible)
    and not atomic adds: the forward image's `exclusive` and, for T / C, the exclusivity proof of the transposed image
    (_common.interpret_image decides the same way), read off the analysis-only twin -- the analysis does not look at the
    device"""
    twin = bsm.synthetic.build(p, device=NODEV, **kw)
    _, rows, _, waves = get_image(twin, timage=True)
    t = bool(np.any(waves["work"] == WORK_SCALE)) or _image_exclusive(waves, rows, p["size"][1])
    return [twin.stats()["exclusive"] == 1, t, t]


@pytest.mark.parametrize("kind", ["blocksparse", "vbcrs"])
@pytest.mark.parametrize("dtype", DTYPES, ids=name_of)
def test_transposed_image_packed_and_refilled(torch_cuda, bsm, kind, dtype):
    """The export does not reach the transposed image, products do (ops T and C of a transpose_image handle run forward
    on it): a device-packed handle and handles built from NaN and refilled compute what a handle fresh from the host
    blocks computes, and no NaN reaches any product.  Bitwise wherever a product is reproducible: every op in mode
    gather, and in mode direct the ops whose image is exclusive (one launch of plain stores).  The other direct-mode
    products add with atomics and are held to the product bounds of test_gpu_fuzz.py (max|.| / max|ref|; a misplaced
    value is an error of the order of the product itself).

    The update tests decide "reproducible" by whether two fresh handles agree bitwise.  On these small operators that is
    chance: atomic adds in another order often give the same bits (blocksparse float32 case 2, op T in mode direct: 7
    distinct results in 12 runs of ONE handle, while two fresh handles happened to agree), so the decision is
    made from the structure, and two fresh handles are required to agree where it says reproducible."""
    torch = torch_cuda
    ops, _ = operators(kind, dtype)
    seed = value_seed(kind, dtype)
    rng = np.random.default_rng(seed + 6)
    tol = TOL[np.dtype(dtype)]
    nprod = nbit = 0
    for case, p in enumerate(ops):
        nr, nc = p["size"]
        xs = [torch.from_numpy(rand_vec(rng, n, dtype)).cuda() for n in (nc, nr, nr)]
        hollow = nan_blocks(p)
        nb = len(src_list(p))
        for acc in ("gather", "direct"):
            kw = dict(accumulate=acc, transpose_image=True)
            bitwise = [True] * 3 if acc == "gather" else exclusive_products(bsm, p, kw)
            fresh = one_column_products(bsm, torch, bsm.synthetic.build(p, **kw), xs)
            again = one_column_products(bsm, torch, bsm.synthetic.build(p, **kw), xs)
            tested = [("device-packed", bsm.synthetic.build(device_blocks(torch, p), **kw))]
            for where in ("host", "device"):
                A = bsm.synthetic.build(hollow if where == "host" else on_device(torch, hollow), **kw)
                ids = np.arange(1, nb + 1) if where == "host" else rng.permutation(nb) + 1  # (in order / the item-list path)
                update(torch, A, ids, [src_list(p)[i - 1] for i in ids], where, 0 if where == "host" else 3)
                tested.append((f"refilled from {where} blocks", A))
            for op, (f, f2) in enumerate(zip(fresh, again)):
                assert not np.any(np.isnan(f)), (seed, case, acc, op)
                assert np.array_equal(f, f2) or not bitwise[op], (seed, case, acc, op, "two fresh handles differ")
            for what, A in tested:
                got = one_column_products(bsm, torch, A, xs)
                for op, (g, f) in enumerate(zip(got, fresh)):
                    assert not np.any(np.isnan(g)), (seed, case, acc, what, op)
                    if bitwise[op]:
                        assert np.array_equal(g, f), (seed, case, acc, what, op, relerr(g, f))
                    else:
                        assert relerr(g, f) < tol, (seed, case, acc, what, op, relerr(g, f))
                    nprod += 1
                    nbit += bitwise[op]
    print(f"VALSTAT transposed {kind} {name_of(dtype)} operators {NOPS} products {nprod} bitwise {nbit}")


# ---- 6. multi-device handles: values only -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=name_of)
def test_values_of_a_multi_device_handle(torch_cuda, bsm, kind, dtype):
    torch = torch_cuda
    ops, refs = operators(kind, dtype)
    seed = value_seed(kind, dtype)
    case = busiest(ops)
    p = ops[case]
    rng = np.random.default_rng(seed + 7)
    total = 0
    for where in ("host", "device"):
        A = bsm.synthetic.build(p if where == "host" else on_device(torch, p), devices=[0, 0, 0])
        check_export(bsm, A, p, refs[case], seed, case, f"{where} blocks over three devices")
        vb = new_values(p, rng)
        ids, blocks, cur = subset_of(rng, p, vb)
        for k, (i, b, pad, q) in enumerate([(range(1, len(vb) + 1), vb, 0, with_values(p, vb)), (ids, blocks, 3, with_values(p, cur))]):
            update(torch, A, i, b, where, pad)
            want = canonical(*coo_triples(q))
            check_export(bsm, A, q, want, seed, case, f"three devices, {where} update {k}")
            total += len(want)
    valstat("multidevice", kind, dtype, 1, total)
