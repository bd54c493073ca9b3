#!/usr/bin/env python3
"""Developer probe: polynomial preconditioners as handles (bsm.chebyshev / bsm.neumann: bsm_poly_create) under the device
solvers, by the window protocol of tools/cg_bench.py -- but every solve runs to a FIXED rtol, because what a polynomial buys
is fewer outer iterations: `reps` timed windows after one warm-up window, each window `solves` solves in a row, host clock
around calls that end in a device synchronise, the variants' windows alternating; [min, median, max].  One JSON line per
(leg, K), build id included; per variant the outer iteration count, ms per solve, ms per outer iteration, the products with
A and with the innermost D one solve issues, and the speed-up over the leg's baseline (medians).
  cg_c3     Cg on C3 (SymmetricBlockMatrix, 200 000 rows, float64, generated in HBM, shifted to definiteness as
            tools/cg_bench.py does): M = block_jacobi(A) against chebyshev(steps = 2, 4, 8, D = block_jacobi(A)) over
            [0.95 lo, 1.05 hi] from lanczos_bounds(A, D, 20), whose cost is reported separately (lanczos_ms)
  gmres_c2  GmresMulti(30) on C2 plus s I on every row segment (tools/bicgstab_bench.py: shifted_c2; C2 itself holds no
            diagonal entries, so no Jacobi D exists for it and GMRES(30) stagnates on it): no preconditioner against
            block_jacobi over the row segments alone and neumann(omega, steps = 2, 4, D = that block_jacobi)
usage: poly_bench.py [--only cg_c3,gmres_c2] [--columns 1,8] [--reps 5] [--solves 5] [--rtol 1e-8] [--omega 1.0]"""
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
from bicgstab_bench import shifted_c2  # noqa: E402
from cg_bench import med, shift_diagonal, spectral_radius, stats, window  # noqa: E402

S = bsm.synthetic


def run_leg(torch, name, make, variants, K, a, extra):
    """variants: label -> M (None: no preconditioner); make(M, K) -> solver.  One JSON line"""
    A = extra["A"]
    n, dt = A.size[0], A.dtype
    B = torch.from_numpy(np.random.default_rng(0xC6).uniform(-1, 1, (K, n)).astype(dt)).cuda().t()  # column-major n x K
    X = torch.empty((K, n), dtype=B.dtype, device="cuda").t()
    solvers = {k: make(M, K) for k, M in variants.items()}
    runs = {k: (lambda s=s: s.solve(B, X=X, rtol=a.rtol, maxiter=a.maxiter)[1]) for k, s in solvers.items()}
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    base = next(iter(runs))
    out = {"leg": name, "build": L.lib().bsm_version().decode().split()[-1], "n": n, "dtype": dt.name, "K": K, "rtol": a.rtol,
           "solves_per_window": a.solves, "windows": a.reps, "baseline": base}
    out.update(extra["record"])
    for k, info in last.items():
        M = variants[k]
        inner = getattr(M, "steps", 1 if M is not None else 0)
        its = int(info.iterations)
        out[k] = {"status": int(info.status), "outer_iterations": its, "ms_per_solve": stats(times[k]),
                  "ms_per_outer_iteration": stats([t / max(its, 1) for t in times[k]]),
                  "a_products": int(info.a_products) + int(info.m_products) * max(inner - 1, 0),
                  "d_products": int(info.m_products) * inner,
                  "speedup_over_baseline": round(med(times[base]) / med(times[k]), 3),
                  "worst_relative_residual": float(np.max(info.residual / info.bnorm))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="cg_c3,gmres_c2")
    ap.add_argument("--columns", default="1,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=5)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=600)
    ap.add_argument("--omega", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    columns = [int(k) for k in a.columns.split(",")]
    if "cg_c3" in a.only.split(","):
        A = S.build(S.config3(on_device=True))
        n, dt = A.size[0], A.dtype
        shift = 1.1 * spectral_radius(torch, A, n, dt)  # the generated operator is indefinite (tools/cg_bench.py)
        shift_diagonal(torch, A, shift)
        D = bsm.block_jacobi(A)
        bsm.lanczos_bounds(A, D, steps=20)  # warm-up
        lz = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            lo, hi = bsm.lanczos_bounds(A, D, steps=20)
            lz.append(time.perf_counter() - t)
        for K in columns:
            variants = {"block_jacobi": D}
            variants.update({f"chebyshev{s}": bsm.chebyshev(A, 0.95 * lo, 1.05 * hi, s, D=D, nrhs=K) for s in (2, 4, 8)})
            run_leg(torch, "cg_c3", lambda M, k: bsm.Cg(A, M, nrhs=k), variants, K, a,
                    {"A": A, "record": {"shift": round(shift, 3), "ritz": [lo, hi], "lanczos_ms": stats(lz)}})
        del A, D, variants
    if "gmres_c2" in a.only.split(","):
        A, shift = shifted_c2(torch, None)
        rstart, rsz = S.config2_row_segments(A.size[0])
        sets = [np.arange(s + 1, s + m + 1, dtype=np.int64) for s, m in zip(rstart, rsz)]
        D = bsm.block_jacobi(A, sets)
        for K in columns:
            variants = {"none": None, "block_jacobi": D}
            variants.update({f"neumann{s}": bsm.neumann(A, a.omega, s, D=D, nrhs=K) for s in (2, 4)})
            run_leg(torch, "gmres_c2", lambda M, k: bsm.GmresMulti(A, M, nrhs=k, restart=30), variants, K, a,
                    {"A": A, "record": {"shift": round(shift, 3), "omega": a.omega}})


if __name__ == "__main__":
    main()
