"""The rank process of the process-per-GPU tests (tests/test_distributed_cpu.py, tests/test_fuzz_distributed_cpu.py,
the fuzz cases of tests/test_gpu_distributed.py): one process group over `gloo`, one or several operators looped inside
it, every leg of blocksparsematrices.jl_amd/distributed.py on each, rank 0 compares the assembled results with the CPU
oracle on the WHOLE operator.

device "cpu": each rank's LOCAL product is executed by the packed-image interpreter of tests/_common.py (the same image
the HIP kernel walks) through the `local_mul` hooks; "cuda": real device handles on cuda:0 and the HIP product.

`source` names the operators:
    "vbcrs", "vbcrs_tiny", "vbcrs_T_across", "vbcrs_cols_T", "blocksparse", "symmetric"   the regular ones
    ("fuzz", kind, dtype name, count, mode)   `count` operators of _fuzz.GEN[kind] from seed_of(kind, dtype);
        mode "square": _fuzz.squared, every leg (complex symmetric: the transposed and adjoint products as well);
        mode "rect": as drawn -- op N with full x, op T across the row partition, and (VBCRS) op T on the column
        partition
"""
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def fuzz_problems(kind, dtype, count):
    from _fuzz import GEN, seed_of
    rng = np.random.default_rng(seed_of(kind, dtype))
    return [GEN[kind](rng, np.dtype(dtype)) for _ in range(count)]


def _problems(source, small):
    """-> [(problem, legs)], legs: "along" (every leg of the product along the row partition), "T_across", "cols_T",
    "ops" (the mul legs under op T and C: symmetric operators), several joined by "+".  small: the sizes of the CPU
    tests (the GPU tests take the regular operators larger)"""
    import bsm_amd as bsm
    if isinstance(source, str):
        legs = {"vbcrs_T_across": "T_across", "vbcrs_cols_T": "cols_T"}.get(source, "along")
        if source == "vbcrs_tiny":  # 2 block rows on 3 ranks: one rank owns nothing and creates no handle
            rng = np.random.default_rng(1)
            prob = dict(kind="vbcrs", blocks=[np.asfortranarray(rng.standard_normal((9, 12))),
                                              np.asfortranarray(rng.standard_normal((7, 5)))],
                        rowstart=np.array([4, 30]), colstart=np.array([2, 20]), size=(40, 40),
                        x=rng.standard_normal(40))
        elif source.startswith("vbcrs"):
            prob = bsm.synthetic.config2(n=5000, nblocks=300) if small else bsm.synthetic.config2(n=20_000, nblocks=900)
        elif source == "blocksparse":
            prob = bsm.synthetic.config1(n=3000, nblocks=120, bs=24)
        else:
            prob = bsm.synthetic.config5(n=5000, lo=16, hi=96, halfband=3) if small else \
                bsm.synthetic.config5(n=60_000, lo=16, hi=128, halfband=3)
        return [(prob, legs)]
    from _common import rand_vec
    from _fuzz import squared
    _, kind, dtype, count, mode = source
    out = []
    for i, p in enumerate(fuzz_problems(kind, dtype, count)):
        p = squared(p) if mode == "square" else p
        p["x"] = rand_vec(np.random.default_rng(100 + i), max(p["size"]), dtype)  # (cut to the length a product reads)
        if mode == "square":
            out.append((p, "along+ops" if kind == "symmetric" and np.dtype(dtype).kind == "c" else "along"))
        else:
            out.append((p, "N+T_across" + ("+cols_T" if kind == "vbcrs" else "")))
    return out


def run(rank, world, port, source, q, device="cpu"):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        if device != "cpu":
            torch.cuda.set_device(0)
        errs, own, touched = [], None, None
        orc = None
        for prob, legs in _problems(source, small=(device == "cpu")):
            res, own, touched = _one_operator(prob, legs.split("+"), rank, world, device, not isinstance(source, str))
            if rank == 0:  # only rank 0 loads (and on a clean tree builds) the oracle
                if orc is None:
                    from oracle import load_oracle
                    orc = load_oracle()
                from _common import oracle_mul, relerr
                for op, x, y0, alpha, beta, got in res:
                    ref = oracle_mul(orc, prob, op, x, y0, alpha, beta, strong=(beta == 0))
                    errs.append(relerr(got, ref))
        if rank == 0:
            q.put(("ok", errs, own, touched))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback
        q.put(("err", traceback.format_exc(), None, None))
        raise


def _one_operator(prob, legs, rank, world, device, fuzz):
    """every leg in `legs` on one operator -> ([(op, x, y0, alpha, beta, assembled result)], own, touched)"""
    import torch
    import torch.distributed as dist
    import bsm_amd as bsm
    from bsm_amd import distributed as D
    from _common import NODEV, Cc, N, T, interpret_image, nblocks

    cpu = device == "cpu"
    kind = prob["kind"]
    sym = kind == "symmetric"
    nr, nc = prob["size"]
    dt = np.dtype(prob["x"].dtype)
    out = []

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t if cpu else t.cuda()

    def host(t):
        if not cpu:
            torch.cuda.synchronize()
        return t.cpu()

    def assemble(t, rng_):
        """test-side assembly of the ranks' slices: rows rng_ of t from this rank, zero elsewhere, summed"""
        t = host(t)
        part = torch.zeros_like(t)
        if rng_[1] >= rng_[0]:
            part[rng_[0] - 1:rng_[1]] = t[rng_[0] - 1:rng_[1]]
        flat = torch.view_as_real(part) if part.is_complex() else part  # (gloo reduces no complex tensors)
        dist.all_reduce(flat)
        return part.numpy().copy()

    def image_mul(H, rows):
        """the interpreter in place of the HIP product of handle H, which writes `rows` (None: all of y) under op N and
        the whole y under op T / C"""
        def f(yy, xx, alpha, beta, lop=N):
            strong = beta is False
            a = 1 if alpha is True else alpha
            b = 0 if strong else (1 if beta is True else beta)
            res = interpret_image(H, lop, xx.numpy(), yy.numpy(), a, b, strong)
            if lop != N or rows is None:
                yy[:] = torch.from_numpy(res)  # transposed products scale the whole y
            else:
                yy[rows[0] - 1:rows[1]] = torch.from_numpy(res[rows[0] - 1:rows[1]])  # the handle's own range
            return yy
        return f

    def split(axis):
        if kind == "vbcrs":
            local, own = D.split_vbcrs(prob, rank, world, axis=axis)
            return local, own, D.touched_range(local, own, axis)
        assert axis == 0
        return D.split_blocksparse(prob, rank, world) if kind == "blocksparse" else D.split_symmetric(prob, rank, world)

    def handle(local, rows):
        """`own` = the rows this handle is responsible for scaling by beta (C ABI bsm_options.own_lo/hi)"""
        if D.is_empty(local):
            return None
        if cpu:
            return bsm.synthetic.build(local, device=NODEV, **({"own": rows} if rows is not None else {}))
        return D.build_local(local, rows)

    scalars = ((True, False), (0.5, -2.0)) if dt.kind != "c" else ((True, False), (0.5 - 0.25j, -2.0 + 0.5j))
    sections = []
    if "along" in legs or "N" in legs:
        sections.append((N, 0, "along" in legs))
    if "ops" in legs:
        sections += [(T, 0, False), (Cc, 0, False)]
    if "T_across" in legs:
        sections.append((T, 0, False))
    if "cols_T" in legs:
        sections.append((T, 1, False))
    local = own = touched = A = None
    for op, axis, full in sections:
        if local is None or axis != 0:
            local, own, touched = split(axis)
            A = handle(local, touched if axis == 0 else None)
        hook = image_mul(A, touched if axis == 0 else None) if cpu and A is not None else None
        xl, yl = (nc, nr) if op == N else (nr, nc)
        xh = prob["x"][:xl].copy()
        x = dev(xh)
        y0 = np.random.default_rng(7).standard_normal(yl).astype(dt)
        along = sym or ((op == N) == (axis == 0))
        for gather in (True, False):
            P = D.RowPartitioned(A, own, touched, gather=gather, axis=axis, symmetric=sym)
            for alpha, beta in scalars:
                y = dev(y0.copy())
                for _ in range(1 if cpu else 2):  # (device: again, on the cached plan / buffers)
                    P.mul(y.copy_(dev(y0)), x, alpha, beta, local_mul=hook, op=op)
                if gather:
                    got = host(y).numpy().copy()
                else:  # only this rank's output range is final
                    got = assemble(y, own if along else P.out_range(yl))
                out.append((op, xh, y0, 1 if alpha is True else alpha, 0 if beta is False else beta, got))
        if not full:
            continue
        n = nr
        a2, b2 = scalars[1]

        def own_only(v):
            """v (a vector or rows x K) valid on the own rows only, NaN elsewhere"""
            d = np.full_like(v, np.nan)
            if own[1] >= own[0]:
                d[own[0] - 1:own[1]] = v[own[0] - 1:own[1]]
            return d
        if kind in ("vbcrs", "symmetric") or fuzz:
            # x and y PARTITIONED like the rows: x is valid on the own range only (NaN elsewhere); the
            # symmetric operator fetches its halo point-to-point, the others all-gather the slices
            P = D.RowPartitioned(A, own, touched, gather=False, symmetric=sym, xneed=touched if sym else None)
            for _ in range(2):
                y = dev(y0.copy())
                P.mul(y, dev(own_only(xh)), a2, b2, x_distributed=True, local_mul=hook)
            out.append((N, xh, y0, a2, b2, assemble(y, own)))
        # the same partitioned-vector product with the exchange OVERLAPPED with the interior rows: two images per rank
        # (interior / boundary blocks, distributed.split_interior), the boundary one on the side of the exchange
        interior, boundary, bt, bx = D.split_interior(local, own)
        assert nblocks(interior) + nblocks(boundary) == nblocks(local)
        if cpu:
            Ai = None if D.is_empty(interior) else bsm.synthetic.build(interior, device=NODEV, own=own)
            Ab = None if D.is_empty(boundary) else bsm.synthetic.build(boundary, device=NODEV, own=bt)
            xmodes = ("halo", "allgather") if kind != "blocksparse" or fuzz else ("allgather",)
        else:
            xmodes = ("halo", "allgather", "auto") if kind != "blocksparse" or fuzz else ("auto",)
        for xmode in xmodes:
            if cpu:
                P = D.RowPartitioned(Ab, own, bt, gather=False, symmetric=sym, xneed=(bx if xmode == "halo" else None),
                                     interior=Ai)
                hooks = dict(local_mul=image_mul(Ab, bt) if Ab is not None else None,
                             interior_mul=image_mul(Ai, own) if Ai is not None else
                             (lambda yy, xx, a, b: P._combine(yy, slice(own[0] - 1, own[1]), 0, b) if own[1] >= own[0] else None))
            else:
                P = D.build_overlapped(local, own, symmetric=sym, xmode=xmode)
                hooks = {}
            for alpha, beta in scalars:
                for _ in range(2 if cpu else 3):  # again: cached plans, reused receive buffers
                    y = dev(y0.copy())
                    P.mul_overlapped(y, dev(own_only(xh)), alpha, beta, **hooks)
                out.append((N, xh, y0, 1 if alpha is True else alpha, 0 if beta is False else beta, assemble(y, own)))
        # A * X, several right-hand sides, X and Y (column-major) PARTITIONED like the rows: mul_multi -- one local product
        # for all columns, the columns of every halo segment in the one batch of the exchange; xneed=None: the x
        # all-gather, gather=True: the Y all-gather, each ONE collective for all columns
        K = 3 if cpu else 6
        Xf = np.stack([xh * (k + 1) + 0.25 * k for k in range(K)], axis=1)
        Y0 = np.stack([np.random.default_rng(11 + k).standard_normal(n).astype(dt) for k in range(K)], axis=1)

        def colmajor(a):
            return dev(a.T).t()

        def multi_hook(YY, XX, alpha, beta):
            for k in range(K):
                hook(YY[:, k], XX[:, k], alpha, beta)
            return YY
        for xneed, gather in [(touched if sym else None, False), (None, True)] + ([(None, False)] if sym else []):
            P = D.RowPartitioned(A, own, touched, gather=gather, symmetric=sym, xneed=xneed)
            Xbuf = dev(np.empty((K, n), dtype=dt))
            plans = []
            # passes 1, 2: X = Xbuf.t(), a new tensor over the same memory each time (the x plan is kept);
            # pass 3: other memory (the x plan is rebuilt)
            for Xb in (Xbuf, Xbuf, torch.empty_like(Xbuf)):
                Xd = Xb.t()
                Xd.copy_(dev(own_only(Xf)))
                Y = colmajor(Y0)
                P.mul_multi(Y, Xd, a2, b2, x_distributed=True, local_mul=(multi_hook if hook is not None else None))
                plans.append(list((P._xplan or {}).values()))
            assert all(a is b for a, b in zip(plans[0], plans[1])), "the x plan was rebuilt for the same memory"
            got = host(Y).numpy().copy() if gather else assemble(Y, own)  # gather: the whole Y on every rank
            for k in range(K):
                out.append((N, Xf[:, k].copy(), Y0[:, k].copy(), a2, b2, got[:, k]))
    return out, own, touched


def spawn(source, world, device="cpu", timeout=240):
    """one process per rank -> (status, errs, own, touched, exit codes); a rank that crashed or did not finish in time is
    reported (status "err" / "timeout"), whatever is left is ended and nothing else is started"""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=run, args=(r, world, port, source, q, device)) for r in range(world)]
    for p in procs:
        p.start()
    import time
    t0, msg = time.monotonic(), None
    while msg is None:
        try:
            msg = q.get(timeout=1)
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                msg = ("err", "a rank exited with %r" % [p.exitcode for p in procs], None, None)
            elif time.monotonic() - t0 > timeout:
                msg = ("timeout", "no result within %d s" % timeout, None, None)
    for p in procs:
        p.join(timeout=120 if msg[0] == "ok" else 5)
        if p.is_alive():
            p.kill()
            p.join()
    return msg + ([p.exitcode for p in procs],)
