#!/usr/bin/env python3
"""Developer probe: restarted GMRES on the device (bsm.Gmres: bsm_gmres_solve) against the SAME algorithm written with
torch ops around bsm.mul -- what a user could do before the solver existed, and the only thing: right-preconditioned
GMRES(30), CGS2 as `V[:, :j + 1].T.conj() @ w` and `w -= V[:, :j + 1] @ h` twice, the norm of w read with .item(), the
Givens rotations on the host.  Both run a fixed 60 iterations (rtol = 0) on operators generated in HBM, float64:
  c2   VariableBlockCompressedRowStorage, 100 000 rows, no preconditioner (the operator offers no diagonal sets)
  c3   SymmetricBlockMatrix, 200 000 rows, M = block_jacobi(A) over its own diagonalindices
Per operator one JSON line, build id included.  `reps` timed windows after one warm-up window, each window `solves`
solves in a row (default 25: 0.1 s and more per window), host clock around calls that end in a device synchronise (the
native solve is synchronous), native and baseline windows alternating; [min, median, max]:
  native_ms_per_it / torch_ms_per_it     a window over its solves x 60 iterations
  pair_us                                one product pair z = M v, w = A z (A alone without M) enqueued back to back, per pair,
                                         from a window of 200 pairs between two synchronises
  native_outside_products                share of the native time outside the products: 1 - 60 * pair / native solve
  orth_gbs_*_lower_bound                 traffic model of the orthogonalisation, 2 passes x (2 (j + 1) + 3) n s bytes
                                         summed over the 60 iterations, over (solve time - 60 * pair): an UPPER bound of
                                         the time the orthogonalisation takes (it also holds the rotations, the scaling,
                                         the restart and the host's share), so a LOWER bound of its rate
  stream_gbs                             bsm_bench_stream over a buffer of the size of V: the bare streaming read
The basis of c2 is 100 000 x 32 x 8 B = 26 MB and of c3 51 MB: both stay resident in the 256 MB memory-side cache
between the passes, so the rates are cache rates, not HBM rates -- as they are in a user's solve of this size.
Kernel time of the orthogonalisation alone, in a run of its own:
  rocprofv3 --kernel-trace --stats -d traces/gmres -- python3 tools/gmres_bench.py --only c2 --reps 1 --no-torch
usage: gmres_bench.py [--only c2,c3] [--reps 5] [--solves 25] [--restart 30] [--iters 60] [--no-torch]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsm_amd as bsm  # noqa: E402
from bsm_amd import _lib as L  # noqa: E402

S = bsm.synthetic
OPS = {"c2": lambda: S.config2(on_device=True), "c3": lambda: S.config3(on_device=True)}


def stats(ts, scale=1e3, digits=4):
    ts = sorted(ts)
    return [round(ts[0] * scale, digits), round(ts[len(ts) // 2] * scale, digits), round(ts[-1] * scale, digits)]


def torch_gmres(torch, A, M, b, restart, iters):
    """the baseline: the method of bsm_gmres_solve, every vector operation a torch op, every scalar through .item()"""
    n = b.numel()
    x = torch.zeros_like(b)
    V = torch.empty(restart + 1, n, dtype=b.dtype, device=b.device).t()  # column-major
    z, w, r = torch.empty_like(b), torch.empty_like(b), b.clone()
    done, est = 0, 0.0
    while done < iters:
        if done:
            r.copy_(b)
            bsm.mul(r, A, x, -1, 1)
        beta = torch.linalg.vector_norm(r).item()
        V[:, 0] = r / beta
        m = min(restart, iters - done)
        H = [[0.0] * (m + 1) for _ in range(m)]  # columns
        cs, sn, g = [0.0] * m, [0.0] * m, [beta] + [0.0] * m
        for j in range(m):
            if M is not None:
                bsm.mul(z, M, V[:, j])
                bsm.mul(w, A, z)
            else:
                bsm.mul(w, A, V[:, j])
            hs = torch.zeros(j + 1, dtype=b.dtype, device=b.device)
            for _ in range(2):
                h = V[:, :j + 1].T.conj() @ w
                w -= V[:, :j + 1] @ h
                hs += h
            hn = torch.linalg.vector_norm(w).item()
            col = hs.tolist() + [hn]
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], cs[i] * col[i + 1] - sn[i] * col[i]
            rr = math.hypot(col[j], hn)
            cs[j], sn[j] = (col[j] / rr, hn / rr) if rr else (1.0, 0.0)
            col[j], col[j + 1] = rr, 0.0
            g[j + 1], g[j] = -sn[j] * g[j], cs[j] * g[j]
            H[j] = col
            est = abs(g[j + 1])
            V[:, j + 1] = w / hn
        y = [0.0] * m
        for i in range(m - 1, -1, -1):
            y[i] = (g[i] - sum(H[c][i] * y[c] for c in range(i + 1, m))) / H[i][i]
        u = V[:, :m] @ torch.tensor(y, dtype=b.dtype, device=b.device)
        if M is not None:
            bsm.mul(x, M, u, 1, 1)
        else:
            x += u
        done += m
    torch.cuda.synchronize()
    return x, est


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c2,c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=25)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    for name in a.only.split(","):
        A = S.build(OPS[name]())
        M = bsm.block_jacobi(A) if hasattr(A, "diagonalindices") else None
        n = A.size[0]
        b = torch.from_numpy(S.vector(0xB5B5, n)).cuda()
        solver = bsm.Gmres(A, M, restart=a.restart)
        out = {"op": name, "build": build_id, "n": n, "dtype": A.dtype.name, "restart": a.restart, "iterations": a.iters, "solves_per_window": a.solves, "windows": a.reps,
               "preconditioner": M is not None}
        # the product pair on its own
        v, z, w = b.clone(), torch.empty_like(b), torch.empty_like(b)

        def pairs(count=200):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(count):
                if M is not None:
                    bsm.mul(z, M, v)
                    bsm.mul(w, A, z)
                else:
                    bsm.mul(w, A, v)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / count
        pairs(20)
        pair = [pairs() for _ in range(a.reps)]
        out["pair_us"] = stats(pair, 1e6, 2)
        nat, tor, est = [], [], {}
        for r in range(a.reps + 1):  # the first round warms up; native and baseline windows alternate
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.solves):
                x, info = solver.solve(b, rtol=0.0, maxiter=a.iters)
            dt = (time.perf_counter() - t) / a.solves
            assert info.iterations == a.iters, info
            est["native"] = info.residual / info.bnorm
            if r:
                nat.append(dt)
            if not a.no_torch:
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.solves):
                    xt, e = torch_gmres(torch, A, M, b, a.restart, a.iters)
                dt = (time.perf_counter() - t) / a.solves
                est["torch"] = e / info.bnorm
                if r:
                    tor.append(dt)
        # traffic model of the orthogonalisation over the cycles of `iters` iterations
        model = sum(2 * (2 * ((i % a.restart) + 1) + 3) * n * A.dtype.itemsize for i in range(a.iters))
        med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
        p = med(pair)
        out["native_ms_per_it"] = stats([t / a.iters for t in nat])
        out["native_outside_products"] = round(1 - a.iters * p / med(nat), 4)
        out["orth_model_bytes"] = model
        out["orth_gbs_native_lower_bound"] = round(model / max(med(nat) - a.iters * p, 1e-9) / 1e9, 1)
        out["relative_estimate_native"] = est["native"]
        out["workspace_bytes"] = info.workspace_bytes
        if tor:
            out["torch_ms_per_it"] = stats([t / a.iters for t in tor])
            out["orth_gbs_torch_lower_bound"] = round(model / max(med(tor) - a.iters * p, 1e-9) / 1e9, 1)
            out["relative_estimate_torch"] = est["torch"]
            out["speedup"] = round(med(tor) / med(nat), 3)
        # the bare streaming read of a buffer of the basis' size
        nbytes = (a.restart + 1) * n * A.dtype.itemsize // 16 * 16
        buf = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
        scratch = torch.zeros((8192 + 64 * ((nbytes // 16 + 2047) // 2048) * 4) // 8, dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def stream(count=50):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(count):
                if L.lib().bsm_bench_stream(C.c_void_p(buf.data_ptr()), nbytes, C.c_void_p(scratch.data_ptr()), scratch.numel() * 8, 0, st):
                    raise RuntimeError("bsm_bench_stream failed")
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / count
        stream(5)
        out["stream_bytes"] = nbytes
        out["stream_gbs"] = round(nbytes / med([stream() for _ in range(a.reps)]) / 1e9, 1)
        print(json.dumps(out), flush=True)
        del solver, A, M
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
