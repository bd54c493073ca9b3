#!/usr/bin/env python3
"""Developer probe: thick-restart Lanczos on the device (bsm.Eigsh: bsm_eigsh_solve) on C3 (the symmetric config, float64),
nev = 4 at ncv = 20, 40 and 128, by the window protocol of tools/cg_bench.py: every solve does a FIXED amount of work (rtol = 0, so
no solve converges; maxcycles = 1 or --cycles; vectors off), `reps` timed windows after one warm-up window, each window
`solves` solves in a row, HOST clock around calls that end in a device synchronise, the variants' windows alternating;
[min, median, max].  One JSON line per ncv, build id included:
  1. Eigsh, one cycle: ncv Lanczos steps and one end-of-cycle copy                                     (step_us = time / ncv)
  2. Eigsh, --cycles cycles: the same plus cycles - 1 restarts (host Jacobi, upload, bsm_krylov_combine in place) and
     (cycles - 1) (ncv - keep) more steps                                  (restart_us = what the extra steps do not explain)
  3. the SAME algorithm composed of torch ops around bsm.mul -- two torch.mv passes per step, the norm and the scale on
     device scalars, numpy eigh and one torch.mm per restart --, one cycle and --cycles cycles   (torch_step_us, torch_restart_us)
  4. the bare one-column product, and with it the share of a one-cycle solve outside the products        (outside_products)
  5. bsm.krylov_combine alone, in place, n x ncv -> keep + 1 columns                                             (combine_us)
NOT measured here: a VBCRS operator (a shifted symmetrised C2 is not cheap to make), other types than float64, an MFMA body
for the combine kernel (none was written).
usage: eigsh_bench.py [--reps 5] [--solves 3] [--cycles 4] [--no-torch]"""
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


def keep_of(nev, ncv):
    return min(ncv - 1, nev + (ncv - nev) // 2)


def torch_eigsh(torch, A, v0, nev, ncv, cycles):
    """the baseline: the recurrences of bsm_eigsh_solve (LA, no convergence test), every vector operation a torch op, one host
    read per cycle"""
    n = v0.numel()
    V = torch.zeros((ncv + 1, n), dtype=v0.dtype, device=v0.device).t()
    V[:, 0] = v0 / torch.linalg.vector_norm(v0)
    keep = keep_of(nev, ncv)
    start, kept, arrow = 0, np.zeros(0), np.zeros(0)
    w = torch.empty(n, dtype=v0.dtype, device=v0.device)
    theta = None
    for _ in range(cycles):
        alpha, beta = [], []
        for j in range(start, ncv):
            bsm.mul(w, A, V[:, j].contiguous())
            Vj = V[:, :j + 1]
            h = torch.mv(Vj.t(), w)
            w -= torch.mv(Vj, h)
            h2 = torch.mv(Vj.t(), w)
            w -= torch.mv(Vj, h2)
            b = torch.linalg.vector_norm(w)
            V[:, j + 1] = w / b
            alpha.append(h[j] + h2[j])
            beta.append(b)
        ab = torch.stack(alpha + beta).cpu().numpy()
        m = ncv - start
        T = np.zeros((ncv, ncv))
        for i in range(start):
            T[i, i] = kept[i]
            T[i, start] = T[start, i] = arrow[i]
        for i in range(m):
            T[start + i, start + i] = ab[i]
            if start + i + 1 < ncv:
                T[start + i, start + i + 1] = T[start + i + 1, start + i] = ab[m + i]
        theta, Sm = np.linalg.eigh(T)
        idx = np.arange(ncv - 1, ncv - 1 - keep, -1)
        kept, arrow = theta[idx], ab[-1] * Sm[ncv - 1, idx]
        Sd = torch.from_numpy(np.ascontiguousarray(Sm[:, idx])).to(v0.device)
        carried = V[:, ncv].clone()
        V[:, :keep] = V[:, :ncv] @ Sd
        V[:, keep] = carried
        start = keep
    torch.cuda.synchronize()
    return theta[-nev:]


def measure(torch, name, A, ncv, a, build_id):
    n = A.size[0]
    rng = np.random.default_rng(0xE1)
    v0 = torch.from_numpy(rng.uniform(-1, 1, n)).cuda()
    E = bsm.Eigsh(A, nev=NEV, ncv=ncv, which="LA")
    keep = keep_of(NEV, ncv)
    kw = dict(rtol=0.0, vectors=False)
    runs = {"eigsh_1": lambda: E.solve(v0, maxcycles=1, **kw)[2], "eigsh_c": lambda: E.solve(v0, maxcycles=a.cycles, **kw)[2]}
    if not a.no_torch:
        runs["torch_1"] = lambda: torch_eigsh(torch, A, v0, NEV, ncv, 1)
        runs["torch_c"] = lambda: torch_eigsh(torch, A, v0, NEV, ncv, a.cycles)
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    x, y = v0.clone(), torch.empty_like(v0)

    def bare(count=50):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            bsm.mul(y, A, x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    bare(5)
    prod = med([bare() for _ in range(a.reps)])
    V = torch.from_numpy(rng.uniform(-1, 1, (ncv + 1, n))).cuda().t()
    Sm = torch.from_numpy(rng.uniform(-1, 1, (keep, ncv))).cuda().t()

    def combine(count=20):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            bsm.krylov_combine(V, Sm, carry=ncv)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    combine(3)
    comb = med([combine() for _ in range(a.reps)])
    extra = (a.cycles - 1) * (ncv - keep)
    out = {"op": name, "build": build_id, "size": [int(n), int(n)], "dtype": A.dtype.name, "kind": type(A).__name__, "nev": NEV, "ncv": ncv,
           "keep": keep, "cycles": a.cycles, "solves_per_window": a.solves, "windows": a.reps, "clock": "host"}
    for tag in ("eigsh", "torch"):
        if tag + "_1" not in times:
            continue
        out[tag + "_one_cycle_ms"] = stats(times[tag + "_1"])
        out[tag + "_cycles_ms"] = stats(times[tag + "_c"])
        step = med(times[tag + "_1"]) / ncv
        out[tag + "_step_us"] = round(step * 1e6, 2)
        out[tag + "_restart_us"] = round((med(times[tag + "_c"]) - med(times[tag + "_1"]) - extra * step) / max(a.cycles - 1, 1) * 1e6, 2)
    out["product_us"] = round(prod * 1e6, 2)
    out["outside_products"] = round(1 - ncv * prod / med(times["eigsh_1"]), 4)
    out["combine_us"] = round(comb * 1e6, 2)
    out["combine_gbytes_per_s"] = round((ncv + 1 + keep + 1) * n * 8 / comb / 1e9, 1)
    if "torch_1" in times:
        out["speedup_over_torch"] = {"one_cycle": round(med(times["torch_1"]) / med(times["eigsh_1"]), 3),
                                     "cycles": round(med(times["torch_c"]) / med(times["eigsh_c"]), 3)}
        out["largest_ritz_values"] = {"eigsh": [float(v) for v in last["eigsh_c"].value], "torch": [float(v) for v in last["torch_c"][::-1]]}
    i1, ic = last["eigsh_1"], last["eigsh_c"]
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
    A = S.build(S.config3())
    for ncv in (20, 40, 128):
        measure(torch, "c3", A, ncv, a, build_id)


if __name__ == "__main__":
    main()
