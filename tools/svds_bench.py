#!/usr/bin/env python3
"""Developer probe: thick-restart Golub-Kahan-Lanczos on the device (bsm.Svds: bsm_svds_solve) on C2 (VBCRS, float64, 100 000 x
100 000) and on C2 stacked on itself (200 000 x 100 000, the operator of tools/lsqr_bench.py), nsv = 4 at ncv = 20 and 40, by the
window protocol of tools/eigsh_bench.py: every solve does a FIXED amount of work (rtol = 0, so no solve converges; maxcycles = 1
or --cycles; vectors off), `reps` timed windows after one warm-up window, each window `solves` solves in a row, HOST clock
around calls that end in a device synchronise, the variants' windows alternating; [min, median, max].  One JSON line per
operator and ncv, build id included:
  1. Svds, one cycle: ncv steps (a forward and an adjoint product each) and one end-of-cycle copy        (step_us = time / ncv)
  2. Svds, --cycles cycles: the same plus cycles - 1 restarts (host Jacobi SVD, two uploads, two bsm_krylov_combine in place)
     and (cycles - 1) (ncv - keep) more steps                               (restart_us = what the extra steps do not explain)
  3. the SAME algorithm composed of torch ops around bsm.mul -- two torch.mv passes per side and step, the norms and the
     scales on device scalars, numpy svd and two torch.mm per restart --, one cycle and --cycles cycles
  4. the two bare one-column products (forward + adjoint), and with them the share of a one-cycle solve outside the products
NOT measured here: other types than float64, a transpose_image handle (the adjoint product of C2 runs the transposed path),
the residual pass (vectors off).
usage: svds_bench.py [--reps 5] [--solves 3] [--cycles 4] [--no-torch]"""
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
from lsqr_bench import tall_of  # noqa: E402

S = bsm.synthetic
NSV = 4


def keep_of(nsv, ncv):
    return min(ncv - 1, nsv + (ncv - nsv) // 2)


def torch_svds(torch, A, AH, v0, nsv, ncv, cycles):
    """the baseline: the recurrences of bsm_svds_solve (LM, no convergence test), every vector operation a torch op, one host
    read per cycle"""
    m, n = bsm.size(A)
    P = torch.zeros((ncv + 1, n), dtype=v0.dtype, device=v0.device).t()
    Q = torch.zeros((ncv, m), dtype=v0.dtype, device=v0.device).t()
    P[:, 0] = v0 / torch.linalg.vector_norm(v0)
    keep = keep_of(nsv, ncv)
    start, kept, arrow = 0, np.zeros(0), np.zeros(0)
    q = torch.empty(m, dtype=v0.dtype, device=v0.device)
    r = torch.empty(n, dtype=v0.dtype, device=v0.device)
    sig = None

    def orth(W, w):
        if W.shape[1]:
            w -= torch.mv(W, torch.mv(W.t(), w))
            w -= torch.mv(W, torch.mv(W.t(), w))
        return torch.linalg.vector_norm(w)
    for _ in range(cycles):
        alpha, beta = [], []
        for j in range(start, ncv):
            bsm.mul(q, A, P[:, j].contiguous())
            a = orth(Q[:, :j], q)
            Q[:, j] = q / a
            bsm.mul(r, AH, Q[:, j].contiguous())
            b = orth(P[:, :j + 1], r)
            P[:, j + 1] = r / b
            alpha.append(a)
            beta.append(b)
        ab = torch.stack(alpha + beta).cpu().numpy()
        k = ncv - start
        Bp = np.zeros((ncv, ncv))
        for i in range(start):
            Bp[i, i] = kept[i]
            Bp[i, start] = arrow[i]
        for i in range(k):
            Bp[start + i, start + i] = ab[i]
            if start + i + 1 < ncv:
                Bp[start + i, start + i + 1] = ab[k + i]
        X, sig, Yt = np.linalg.svd(Bp)
        idx = np.arange(keep)
        kept, arrow = sig[idx], ab[-1] * X[ncv - 1, idx]
        Yd = torch.from_numpy(np.ascontiguousarray(Yt.T[:, idx])).to(v0.device)
        Xd = torch.from_numpy(np.ascontiguousarray(X[:, idx])).to(v0.device)
        carried = P[:, ncv].clone()
        P[:, :keep] = P[:, :ncv] @ Yd
        P[:, keep] = carried
        Q[:, :keep] = Q[:, :ncv] @ Xd
        start = keep
    torch.cuda.synchronize()
    return sig[:nsv]


def measure(torch, name, A, ncv, a, build_id):
    m, n = A.size
    AH = bsm.adjoint(A)
    rng = np.random.default_rng(0x5D)
    v0 = torch.from_numpy(rng.uniform(-1, 1, n)).cuda()
    E = bsm.Svds(A, nsv=NSV, ncv=ncv, which="LM")
    keep = keep_of(NSV, ncv)
    kw = dict(rtol=0.0, vectors=False)
    runs = {"svds_1": lambda: E.solve(v0, maxcycles=1, **kw)[3], "svds_c": lambda: E.solve(v0, maxcycles=a.cycles, **kw)[3]}
    if not a.no_torch:
        runs["torch_1"] = lambda: torch_svds(torch, A, AH, v0, NSV, ncv, 1)
        runs["torch_c"] = lambda: torch_svds(torch, A, AH, v0, NSV, ncv, a.cycles)
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    x, y = v0.clone(), torch.empty(m, dtype=v0.dtype, device="cuda")

    def bare(count=50):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            bsm.mul(y, A, x)
            bsm.mul(x, AH, y)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    y.zero_()
    x.zero_()  # (zeros stay zeros: the pair can be repeated without overflow)
    bare(5)
    prod = med([bare() for _ in range(a.reps)])
    extra = (a.cycles - 1) * (ncv - keep)
    out = {"op": name, "build": build_id, "size": [int(m), int(n)], "dtype": A.dtype.name, "kind": type(A).__name__, "nsv": NSV, "ncv": ncv,
           "keep": keep, "cycles": a.cycles, "solves_per_window": a.solves, "windows": a.reps, "clock": "host"}
    for tag in ("svds", "torch"):
        if tag + "_1" not in times:
            continue
        out[tag + "_one_cycle_ms"] = stats(times[tag + "_1"])
        out[tag + "_cycles_ms"] = stats(times[tag + "_c"])
        step = med(times[tag + "_1"]) / ncv
        out[tag + "_step_us"] = round(step * 1e6, 2)
        out[tag + "_restart_us"] = round((med(times[tag + "_c"]) - med(times[tag + "_1"]) - extra * step) / max(a.cycles - 1, 1) * 1e6, 2)
    out["product_pair_us"] = round(prod * 1e6, 2)
    out["outside_products"] = round(1 - ncv * prod / med(times["svds_1"]), 4)
    if "torch_1" in times:
        out["speedup_over_torch"] = {"one_cycle": round(med(times["torch_1"]) / med(times["svds_1"]), 3),
                                     "cycles": round(med(times["torch_c"]) / med(times["svds_c"]), 3)}
        out["largest_values"] = {"svds": [float(v) for v in last["svds_c"].value], "torch": [float(v) for v in last["torch_c"]]}
    i1, ic = last["svds_1"], last["svds_c"]
    out["status"], out["a_products"], out["workspace_bytes"] = [int(i1.status), int(ic.status)], [int(i1.a_products), int(ic.a_products)], int(ic.workspace_bytes)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=4)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    p = S.config2()
    for name, prob in (("c2", p), ("c2_tall", tall_of(p, p))):
        A = S.build(prob)
        for ncv in (20, 40):
            measure(torch, name, A, ncv, a, build_id)


if __name__ == "__main__":
    main()
