#!/usr/bin/env python3
"""Developer probe: LSQR on the device (bsm.Lsqr: bsm_lsqr_solve) on C2 (square VBCRS, float64) and on a RECTANGULAR VBCRS
of the same generator with twice as many block rows as block columns (the blocks of C2 stacked on themselves), by the window
protocol of tools/minres_bench.py: every solve runs a fixed count of iterations (rtol = ntol = 0, maxiter = --iters); `reps`
timed windows after one warm-up window, each window `solves` solves in a row, HOST clock around calls that end in a device
synchronise, the variants' windows alternating; [min, median, max] per lockstep iteration.  One JSON line per operator,
build id included.  At K = 1, 8 and 16:
  1. Lsqr                                                                                          (lsqr_k*_ms_per_it)
  2. the SAME recurrences composed of torch ops around bsm.mul with .item() for the scalars, K = 1   (torch_ms_per_it)
  3. the two bare multi-column products (op N + op C) of one iteration, and with them the share of an iteration outside
     the products                                                              (pair_us_k*, k*_outside_products)
usage: lsqr_bench.py [--reps 5] [--solves 5] [--iters 40] [--no-torch]"""
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


def tall_of(p, q):
    """the blocks of two square VBCRS problems of one generator stacked: twice the block rows over the same block columns"""
    m, n = p["size"]
    return dict(kind="vbcrs", blocks=list(p["blocks"]) + list(q["blocks"]), rowstart=np.concatenate([p["rowstart"], q["rowstart"] + m]),
                colstart=np.concatenate([p["colstart"], q["colstart"]]), size=(2 * m, n))


def torch_lsqr(torch, A, b, n, iters):
    """the baseline: the recurrences of bsm_lsqr_solve, every vector operation a torch op, every scalar through .item()"""
    AH = bsm.adjoint(A)
    u, x = b.clone(), torch.zeros(n, dtype=b.dtype, device=b.device)
    v, q = torch.empty_like(x), torch.empty_like(b)
    beta = torch.linalg.vector_norm(u).item()
    bsm.mul(v, AH, u)
    v.div_(beta)
    alpha = torch.linalg.vector_norm(v).item()
    w, p = v / alpha, torch.empty_like(x)
    phibar, rhobar, rnorm = beta, alpha, beta
    for _ in range(iters):
        bsm.mul(q, A, v)
        u.mul_(-alpha / beta).add_(q, alpha=1 / alpha)
        bn = torch.linalg.vector_norm(u).item()
        bsm.mul(p, AH, u)
        v.mul_(-bn / alpha).add_(p, alpha=1 / bn)
        an = torch.linalg.vector_norm(v).item()
        rho = (rhobar * rhobar + bn * bn) ** 0.5
        c, s = rhobar / rho, bn / rho
        theta, rhobar, phi = s * an, -c * an, c * phibar
        phibar = s * phibar
        x.add_(w, alpha=phi / rho)
        w.mul_(-theta / rho).add_(v, alpha=1 / an)
        alpha, beta, rnorm = an, bn, abs(phibar)
    torch.cuda.synchronize()
    return x, rnorm


def measure(torch, name, A, a, build_id):
    m, n = A.size
    dt = A.dtype
    rng = np.random.default_rng(0xC7)
    B = torch.from_numpy(rng.uniform(-1, 1, (16, m)).astype(dt)).cuda().t()  # column-major m x 16
    X = torch.empty((16, n), dtype=B.dtype, device="cuda").t()
    Q = torch.empty((16, m), dtype=B.dtype, device="cuda").t()
    kw = dict(rtol=0.0, ntol=0.0, maxiter=a.iters, history=False)
    solvers = {k: bsm.Lsqr(A, nrhs=k) for k in (1, 8, 16)}
    b, x = B[:, 0].contiguous(), torch.empty(n, dtype=B.dtype, device="cuda")
    runs = {"lsqr_k1": lambda: solvers[1].solve(b, X=x, **kw)[1]}
    for k in (8, 16):
        runs[f"lsqr_k{k}"] = lambda k=k: solvers[k].solve(B[:, :k], X=X[:, :k], **kw)[1]
    if not a.no_torch:
        runs["torch"] = lambda: torch_lsqr(torch, A, b, n, a.iters)
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    AH = bsm.adjoint(A)

    P = torch.empty((16, n), dtype=B.dtype, device="cuda").t()

    def pair(k, count=50):
        # (the inputs stay what they are: the products write Q and P, so nothing grows from round to round)
        xs, us, qs, ps = (x, b, Q[:, 0], P[:, 0]) if k == 1 else (X[:, :k], B[:, :k], Q[:, :k], P[:, :k])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            bsm.mul(qs, A, xs)
            bsm.mul(ps, AH, us)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    X.uniform_(-1, 1)
    x.uniform_(-1, 1)
    out = {"op": name, "build": build_id, "size": [int(m), int(n)], "dtype": dt.name, "kind": type(A).__name__, "iterations": a.iters,
           "solves_per_window": a.solves, "windows": a.reps, "clock": "host"}
    for k in times:
        out[k + "_ms_per_it"] = stats([t / a.iters for t in times[k]])
    for k in (1, 8, 16):
        pair(k, 5)
        pr = med([pair(k) for _ in range(a.reps)])
        out[f"pair_us_k{k}"] = round(pr * 1e6, 2)
        out[f"k{k}_outside_products"] = round(1 - a.iters * pr / med(times[f"lsqr_k{k}"]), 4)
        info = last[f"lsqr_k{k}"]
        out[f"status_k{k}"] = sorted(set(info.column_status.tolist()))
        out[f"products_k{k}"] = int(info.a_products)
    if "torch" in times:
        out["speedup_over_torch"] = round(med(times["torch"]) / med(times["lsqr_k1"]), 3)
        i1 = last["lsqr_k1"]
        out["relative_residual"] = {"lsqr_k1": float(i1.residual[0] / i1.bnorm[0]), "torch": float(last["torch"][1] / i1.bnorm[0])}
    out["workspace_bytes"] = {f"k{k}": int(last[f"lsqr_k{k}"].workspace_bytes) for k in (1, 8, 16)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    p = S.config2()
    measure(torch, "c2", S.build(p), a, build_id)
    measure(torch, "c2_tall", S.build(tall_of(p, p)), a, build_id)


if __name__ == "__main__":
    main()
