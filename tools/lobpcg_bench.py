#!/usr/bin/env python3
"""Developer probe: LOBPCG on the device (bsm.Lobpcg: bsm_lobpcg_solve) on C3 (the symmetric config, float64), nev = 4 at block 8
and 16, with and without block_jacobi(A) as M, beside bsm.Eigsh at ncv 20 and 40, by the window protocol of tools/cg_bench.py:
HOST clock around calls that end in a device synchronise, `reps` timed windows after one warm-up window, the variants' windows
alternating; [min, median, max].  One JSON line per (block, M), build id included:
  1. FIXED work: rtol = 0 and maxiter = --iters / 2 --iters, so no solve converges          (iteration_us = the difference / iters)
  2. the parts of an iteration, each alone in a loop of its own: the block product (bsm.mul on n x block; with M the product
     with M too), ONE block_gram of S (3 block columns) against [S | AS] (6 block), the TWO in-place block_combine (3 block ->
     2 block columns); what is left -- the residual pass, the host Rayleigh-Ritz, the copies and the synchronisation -- is
     `rest_us`.  Bytes per second: the Gram reads 9 block columns, a combine reads 3 block and writes 2 block.
  3. to a tolerance: which = "LA", rtol = --rtol: iterations, products and wall time of Lobpcg, cycles, products and wall time
     of Eigsh at ncv 20 and 40 (one-column products there, block-column products here).
NOT measured here: other types than float64, a VBCRS operator, the residual pass alone (it has no entry point of its own).
usage: lobpcg_bench.py [--reps 5] [--solves 2] [--iters 10] [--rtol 1e-6] [--no-eigsh]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import bsm_amd as bsm  # noqa: E402
from bsm_amd import _lib as L  # noqa: E402
from cg_bench import med, stats, window  # noqa: E402

S = bsm.synthetic
NEV = 4


def loop_us(torch, fn, count, reps):
    def once():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    once()
    return med([once() for _ in range(reps)]) * 1e6


def measure(torch, name, A, M, block, a, build_id):
    n = A.size[0]
    rng = np.random.default_rng(0x10B)
    X0 = torch.from_numpy(rng.uniform(-1, 1, (block, n))).cuda().t()
    E = bsm.Lobpcg(A, nev=NEV, block=block, M=M, which="LA")
    runs = {"short": lambda: E.solve(X0, rtol=0.0, maxiter=a.iters, history=False)[2],
            "long": lambda: E.solve(X0, rtol=0.0, maxiter=2 * a.iters, history=False)[2]}
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    it_us = (med(times["long"]) - med(times["short"])) / a.iters * 1e6
    Y = torch.empty((block, n), dtype=torch.float64, device="cuda").t()
    prod = loop_us(torch, lambda: bsm.mul(Y, A, X0), 20, a.reps)
    mprod = loop_us(torch, lambda: bsm.mul(Y, M, X0), 20, a.reps) if M is not None else 0.0
    Z = torch.from_numpy(rng.uniform(-1, 1, (6 * block, n))).cuda().t()
    G = torch.empty((6 * block, 3 * block), dtype=torch.float64, device="cuda").t()
    work = torch.empty(bsm.block_gram_work(np.float64, n, 3 * block, 6 * block), dtype=torch.uint8, device="cuda")
    gram = loop_us(torch, lambda: bsm.block_gram(Z[:, :3 * block], Z, out=G, work=work), 20, a.reps)
    CC = torch.from_numpy(rng.uniform(-1, 1, (2 * block, 3 * block)) / (3 * block)).cuda().t()
    comb = loop_us(torch, lambda: bsm.block_combine(Z[:, :3 * block], CC), 20, a.reps)
    out = {"op": name, "build": build_id, "size": [int(n), int(n)], "dtype": "float64", "nev": NEV, "block": block, "M": M is not None,
           "iters": a.iters, "solves_per_window": a.solves, "windows": a.reps, "clock": "host",
           "short_ms": stats(times["short"]), "long_ms": stats(times["long"]), "iteration_us": round(it_us, 1),
           "product_us": round(prod, 1), "m_product_us": round(mprod, 1), "gram_us": round(gram, 1), "two_combines_us": round(2 * comb, 1),
           "rest_us": round(it_us - prod - mprod - gram - 2 * comb, 1),
           "gram_gbytes_per_s": round(9 * block * n * 8 / gram / 1e3, 1), "combine_gbytes_per_s": round(5 * block * n * 8 / comb / 1e3, 1),
           "status": [int(last["short"].status), int(last["long"].status)], "workspace_bytes": int(last["long"].workspace_bytes)}
    t = time.perf_counter()
    w, _, info = E.solve(X0, rtol=a.rtol, maxiter=a.maxiter)
    out["to_rtol"] = {"rtol": a.rtol, "status": int(info.status), "iterations": int(info.iterations), "a_products": int(info.a_products),
                      "m_products": int(info.m_products), "drops": int(info.drops), "wall_ms": round((time.perf_counter() - t) * 1e3, 2),
                      "values": [float(v) for v in w], "max_true_residual_over_anorm": float(np.max(info.residual) / info.anorm)}
    print(json.dumps(out), flush=True)


def eigsh_to_rtol(torch, name, A, ncv, a, build_id):
    n = A.size[0]
    v0 = torch.from_numpy(np.random.default_rng(0x10B).uniform(-1, 1, n)).cuda()
    E = bsm.Eigsh(A, nev=NEV, ncv=ncv, which="LA")
    E.solve(v0, rtol=a.rtol, maxcycles=1)
    t = time.perf_counter()
    w, _, info = E.solve(v0, rtol=a.rtol, maxcycles=2000)
    print(json.dumps({"op": name, "build": build_id, "solver": "eigsh", "ncv": ncv, "rtol": a.rtol, "status": int(info.status),
                      "cycles": int(info.cycles), "a_products": int(info.a_products), "wall_ms": round((time.perf_counter() - t) * 1e3, 2),
                      "values": [float(v) for v in w]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--maxiter", type=int, default=500)
    ap.add_argument("--no-eigsh", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    A = S.build(S.config3())
    M = bsm.block_jacobi(A)
    for block in (8, 16):
        for m in (None, M):
            measure(torch, "c3", A, m, block, a, build_id)
    if not a.no_eigsh:
        for ncv in (20, 40):
            eigsh_to_rtol(torch, "c3", A, ncv, a, build_id)


if __name__ == "__main__":
    main()
