#!/usr/bin/env python3
"""Developer probe: restarted GMRES on several right-hand sides in lockstep (bsm.GmresMulti: bsm_gmres_multi_solve) on the
shifted C3-shaped nonsymmetric BlockSparseMatrix of tools/bicgstab_bench.py with block-Jacobi, float64, GMRES(--restart),
by the window protocol of tools/cg_bench.py: every solve runs a fixed count of iterations (rtol = 0, maxiter = --iters);
`reps` timed windows after one warm-up window, each window `solves` solves in a row, host clock around calls that end in
a device synchronise, the variants' windows alternating; [min, median, max] per lockstep iteration.  One JSON line, build
id included:
  1. GmresMulti K = 1 against Gmres: what moving the decisions to the device costs     (multi_k1_ms_per_it / gmres_ms_per_it)
  2. K = 8 in one GmresMulti against 8 Gmres solves -- the acceptance figure: the two [min, max] intervals must not
     overlap                                              (multi_k8_ms_per_it / gmres_x8_ms_per_it, intervals_disjoint)
  3. per A product: GmresMulti K = 8 (one per iteration) against BiCgStab K = 8 (two per iteration)
  4. the workspaces, and the share of a K = 8 iteration outside the products (the bare pair A X, M X timed on its own): the
     orthogonalisation, which every column does for itself, with gm_hess, gm_scale and the records inside it
usage: gmres_multi_bench.py [--reps 5] [--solves 10] [--iters 60] [--restart 30] [--shift auto|S] [--nseg 3125]"""
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
from bicgstab_bench import band_blocksparse  # noqa: E402
from cg_bench import med, stats, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--shift", default="auto")
    ap.add_argument("--nseg", type=int, default=3125)
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    A, sets, shift = band_blocksparse(torch, None if a.shift == "auto" else float(a.shift), nseg=a.nseg)
    M = bsm.block_jacobi(A, sets)
    n, dt = A.size[0], A.dtype
    rng = np.random.default_rng(0xB1C6)
    B = torch.from_numpy(rng.uniform(-1, 1, (8, n)).astype(dt)).cuda().t()  # column-major n x 8
    b = B[:, 0].contiguous()
    X = torch.empty((8, n), dtype=B.dtype, device="cuda").t()
    x = torch.empty_like(b)
    g = bsm.Gmres(A, M, restart=a.restart)
    m1, m8 = bsm.GmresMulti(A, M, nrhs=1, restart=a.restart), bsm.GmresMulti(A, M, nrhs=8, restart=a.restart)
    s8 = bsm.BiCgStab(A, M, nrhs=8)
    kw = dict(rtol=0.0, maxiter=a.iters)

    def gmres_x8():
        for c in range(8):
            info = g.solve(B[:, c].contiguous(), x=x, **kw)[1]
        return info
    runs = {"gmres": lambda: g.solve(b, x=x, **kw)[1], "multi_k1": lambda: m1.solve(b, X=x, **kw)[1],
            "multi_k8": lambda: m8.solve(B, X=X, **kw)[1], "gmres_x8": gmres_x8, "bicgstab_k8": lambda: s8.solve(B, X=X, **kw)[1]}
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    Y8 = torch.empty((8, n), dtype=B.dtype, device="cuda").t()

    def pairs(count=100):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            bsm.mul(Y8, M, B)
            bsm.mul(Y8, A, B)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    pairs(10)
    p8 = med([pairs() for _ in range(a.reps)])
    out = {"op": "c3", "build": build_id, "n": n, "dtype": dt.name, "kind": type(A).__name__, "restart": a.restart, "iterations": a.iters,
           "solves_per_window": a.solves, "windows": a.reps, "shift": round(shift, 3)}
    for k in times:
        out[k + "_ms_per_it"] = stats([t / a.iters for t in times[k]])
    i1, i8 = last["multi_k1"], last["multi_k8"]
    out["status"] = {"multi_k1": i1.column_status.tolist(), "multi_k8": i8.column_status.tolist(), "gmres": int(last["gmres"].status)}
    out["relative_estimate"] = {"gmres": float(last["gmres"].residual / last["gmres"].bnorm), "multi_k1": float(i1.residual[0] / i1.bnorm[0]),
                                "multi_k8_column_0": float(i8.residual[0] / i8.bnorm[0])}
    out["products"] = {"multi_k8": [int(i8.a_products), int(i8.m_products)], "gmres": [int(last["gmres"].a_products), int(last["gmres"].m_products)]}
    out["multi_k1_over_gmres"] = round(med(times["multi_k1"]) / med(times["gmres"]), 3)
    out["speedup_k8_over_8_gmres"] = round(med(times["gmres_x8"]) / med(times["multi_k8"]), 3)
    out["intervals_disjoint"] = bool(max(times["multi_k8"]) < min(times["gmres_x8"]))
    out["k8_in_k1_iterations"] = round(med(times["multi_k8"]) / med(times["multi_k1"]), 3)
    out["gmres_k8_over_bicgstab_k8_per_a_product"] = round(2 * med(times["multi_k8"]) / med(times["bicgstab_k8"]), 3)
    out["pair_us_k8"] = round(p8 * 1e6, 2)
    out["k8_outside_products"] = round(1 - a.iters * p8 / med(times["multi_k8"]), 4)
    out["workspace_bytes"] = {"gmres": int(last["gmres"].workspace_bytes), "multi_k1": int(i1.workspace_bytes),
                              "multi_k8": int(i8.workspace_bytes), "bicgstab_k8": int(last["bicgstab_k8"].workspace_bytes)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
