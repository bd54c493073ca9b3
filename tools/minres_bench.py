#!/usr/bin/env python3
"""Developer probe: MINRES on the device (bsm.Minres: bsm_minres_solve) on a shifted C3-shaped symmetric INDEFINITE
operator, float64, by the window protocol of tools/gmres_multi_bench.py: every solve runs a fixed count of iterations
(rtol = 0, maxiter = --iters); `reps` timed windows after one warm-up window, each window `solves` solves in a row, HOST
clock around calls that end in a device synchronise, the variants' windows alternating; [min, median, max] per lockstep
iteration.  One JSON line, build id included.
The operators.  C3 as generated (SymmetricBlockMatrix, 200 000 rows, in HBM) has a spectrum on both sides of zero
(docs/experiments_r22.md).  P = C3 + 1.1 rho I, rho an estimate of its spectral radius, is the definite sibling
tools/cg_bench.py times CG on; A = C3 + --indef x rho I (default 0.3) is the indefinite operator.  lambda_min / lambda_max of
A are estimated by power iterations on A and on lambda_max I - A and recorded: the run refuses an A that is not indefinite.
M = block_jacobi(P) over its diagonalindices, positive definite.
  1. Minres K = 1 on (A, M) against Cg K = 1 on (P, M): the same two products per iteration, so the difference is the
     vector work                                                             (minres_k1_ms_per_it / cg_k1_ms_per_it)
  2. Minres K = 1 against the SAME recurrences composed of torch ops around bsm.mul with .item() for the scalars
                                                                                                   (torch_ms_per_it)
  3. K = 8 in one Minres against 8 solves with K = 1 on the same solver object -- the expectation from CG is that the two
     [min, max] intervals are disjoint                    (minres_k8_ms_per_it / minres_k1x8_ms_per_it, intervals_disjoint)
  4. the same without M (nom_*), the share of an iteration outside the products (the bare pair A X, M X timed on its own)
     and the workspaces against Cg and GmresMulti(30)
usage: minres_bench.py [--reps 5] [--solves 10] [--iters 60] [--indef 0.3] [--no-torch]"""
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
from cg_bench import med, shift_diagonal, spectral_radius, stats, window  # noqa: E402

S = bsm.synthetic


def extreme_eigenvalues(torch, A, n, dt, its=60):
    """(lambda_min, lambda_max) of the symmetric A, roughly: the eigenvalue of largest modulus by power iteration with a
    Rayleigh quotient, then the other end of the spectrum by power iteration on that eigenvalue times I minus A"""
    def power(apply):
        v = torch.from_numpy(np.random.default_rng(11).uniform(-1, 1, n).astype(dt)).cuda()
        w = torch.empty_like(v)
        lam = 0.0
        for _ in range(its):
            v = v / torch.linalg.vector_norm(v)
            apply(w, v)
            lam = torch.dot(v, w).item()
            v, w = w, v
        return lam
    far = power(lambda w, v: bsm.mul(w, A, v))

    def shifted(w, v):
        bsm.mul(w, A, v)
        w.mul_(-1).add_(v, alpha=far)
    other = far - power(shifted)
    return min(far, other), max(far, other)


def torch_minres(torch, A, M, b, iters):
    """the baseline: the recurrences of bsm_minres_solve, every vector operation a torch op, every scalar through .item()"""
    x, r, v = torch.zeros_like(b), b.clone(), b.clone()
    vo, w, wo, q = torch.zeros_like(b), torch.zeros_like(b), torch.zeros_like(b), torch.empty_like(b)
    z, zn = torch.empty_like(b), torch.empty_like(b)
    if M is not None:
        bsm.mul(z, M, v)
    else:
        z = v
    gam = torch.dot(v, z).item() ** 0.5
    go, eta, s, so, c, co, rn = 1.0, gam, 0.0, 0.0, 1.0, 1.0, 0.0
    for _ in range(iters):
        bsm.mul(q, A, z)
        delta = torch.dot(z, q).item() / gam ** 2
        vo.mul_(-gam / go).add_(q, alpha=1 / gam).sub_(v, alpha=delta / gam)  # v_new in the storage of v_old
        if M is not None:
            bsm.mul(zn, M, vo)
        else:
            zn = vo
        gn = torch.dot(vo, zn).item() ** 0.5
        a0 = c * delta - co * s * gam
        a1 = (a0 * a0 + gn * gn) ** 0.5
        a2, a3 = s * delta + co * c * gam, so * gam
        cn, sn = a0 / a1, gn / a1
        wo.mul_(-a3 / a1).add_(z, alpha=1 / (gam * a1)).sub_(w, alpha=a2 / a1)  # w_new in the storage of w_old
        x.add_(wo, alpha=cn * eta)
        en = -sn * eta
        r.mul_(sn * sn).add_(vo, alpha=cn * en / gn)
        rn = torch.linalg.vector_norm(r).item()
        v, vo, w, wo = vo, v, wo, w
        if M is not None:
            z, zn = zn, z
        else:
            z = v
        go, gam, eta, co, c, so, s = gam, gn, en, c, cn, s, sn
    torch.cuda.synchronize()
    return x, rn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--indef", type=float, default=0.3)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    A, P = S.build(S.config3(on_device=True)), S.build(S.config3(on_device=True))
    n, dt = A.size[0], A.dtype
    rho = spectral_radius(torch, A, n, dt)
    shift_diagonal(torch, P, 1.1 * rho)
    shift_diagonal(torch, A, a.indef * rho)
    lmin, lmax = extreme_eigenvalues(torch, A, n, dt)
    if not lmin < 0 < lmax:
        raise SystemExit(f"A is not indefinite: lambda_min {lmin:.4g}, lambda_max {lmax:.4g}; choose another --indef")
    M = bsm.block_jacobi(P)
    rng = np.random.default_rng(0xC6)
    B = torch.from_numpy(rng.uniform(-1, 1, (8, n)).astype(dt)).cuda().t()  # column-major n x 8
    b = B[:, 0].contiguous()
    X = torch.empty((8, n), dtype=B.dtype, device="cuda").t()
    x = torch.empty_like(b)
    kw = dict(rtol=0.0, maxiter=a.iters)
    m1, m8 = bsm.Minres(A, M, nrhs=1), bsm.Minres(A, M, nrhs=8)
    u1, u8 = bsm.Minres(A, nrhs=1), bsm.Minres(A, nrhs=8)
    c1 = bsm.Cg(P, M, nrhs=1)

    def x8(solver):
        def run():
            for c in range(8):
                info = solver.solve(B[:, c:c + 1], X=X[:, c:c + 1], **kw)[1]
            return info
        return run
    runs = {"minres_k1": lambda: m1.solve(b, X=x, **kw)[1], "cg_k1": lambda: c1.solve(b, X=x, **kw)[1],
            "minres_k8": lambda: m8.solve(B, X=X, **kw)[1], "minres_k1x8": x8(m8),
            "nom_minres_k1": lambda: u1.solve(b, X=x, **kw)[1], "nom_minres_k8": lambda: u8.solve(B, X=X, **kw)[1], "nom_minres_k1x8": x8(u8)}
    if not a.no_torch:
        runs["torch"] = lambda: torch_minres(torch, A, M, b, a.iters)
    times, last = {k: [] for k in runs}, {}
    for r in range(a.reps + 1):  # the first round warms up; the windows alternate
        for k, fn in runs.items():
            dtm, last[k] = window(torch, fn, a.solves)
            if r:
                times[k].append(dtm)
    y1, Y8 = torch.empty_like(b), torch.empty((8, n), dtype=B.dtype, device="cuda").t()

    def products(xs, ys, with_m, count=100):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            bsm.mul(ys, A, xs)
            if with_m:
                bsm.mul(ys, M, xs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count
    prod = {}
    for key, xs, ys, with_m in (("k1", b, y1, True), ("k8", B, Y8, True), ("nom_k1", b, y1, False), ("nom_k8", B, Y8, False)):
        products(xs, ys, with_m, 10)
        prod[key] = med([products(xs, ys, with_m) for _ in range(a.reps)])
    i1, i8 = last["minres_k1"], last["minres_k8"]
    out = {"op": "c3", "build": build_id, "n": n, "dtype": dt.name, "kind": type(A).__name__, "iterations": a.iters,
           "solves_per_window": a.solves, "windows": a.reps, "clock": "host", "rho": round(rho, 3), "shift_A": round(a.indef * rho, 3),
           "shift_P": round(1.1 * rho, 3), "lambda_min": round(lmin, 3), "lambda_max": round(lmax, 3)}
    for k in times:
        out[k + "_ms_per_it"] = stats([t / a.iters for t in times[k]])
    out["status"] = {"minres_k1": i1.column_status.tolist(), "minres_k8": i8.column_status.tolist(), "cg_k1": last["cg_k1"].column_status.tolist(),
                     "nom_minres_k8": last["nom_minres_k8"].column_status.tolist()}
    out["relative_residual"] = {"minres_k1": float(i1.residual[0] / i1.bnorm[0]), "cg_k1_on_P": float(last["cg_k1"].residual[0] / last["cg_k1"].bnorm[0]),
                                "nom_minres_k1": float(last["nom_minres_k1"].residual[0] / last["nom_minres_k1"].bnorm[0])}
    out["products"] = {"minres_k8": [int(i8.a_products), int(i8.m_products)], "cg_k1": [int(last["cg_k1"].a_products), int(last["cg_k1"].m_products)]}
    out["minres_k1_over_cg_k1"] = round(med(times["minres_k1"]) / med(times["cg_k1"]), 3)
    for pre in ("", "nom_"):
        k8, k1x8 = times[pre + "minres_k8"], times[pre + "minres_k1x8"]
        out[pre + "speedup_k8_over_8_k1"] = round(med(k1x8) / med(k8), 3)
        out[pre + "intervals_disjoint"] = bool(max(k8) < min(k1x8))
        out[pre + "pair_us_k1"], out[pre + "pair_us_k8"] = round(prod[pre + "k1"] * 1e6, 2), round(prod[pre + "k8"] * 1e6, 2)
        out[pre + "k1_outside_products"] = round(1 - a.iters * prod[pre + "k1"] / med(times[pre + "minres_k1"]), 4)
        out[pre + "k8_outside_products"] = round(1 - a.iters * prod[pre + "k8"] / med(k8), 4)
    if "torch" in times:
        out["relative_residual"]["torch"] = float(last["torch"][1] / i1.bnorm[0])
        out["speedup_over_torch"] = round(med(times["torch"]) / med(times["minres_k1"]), 3)
    g8 = bsm.GmresMulti(A, M, nrhs=8, restart=30)
    gi = g8.solve(B, X=X, rtol=0.0, maxiter=1)[1]
    ci = bsm.Cg(P, M, nrhs=8).solve(B, X=X, rtol=0.0, maxiter=1)[1]
    out["workspace_bytes"] = {"minres_k1": int(i1.workspace_bytes), "minres_k8": int(i8.workspace_bytes), "nom_minres_k8": int(last["nom_minres_k8"].workspace_bytes),
                              "cg_k1": int(last["cg_k1"].workspace_bytes), "cg_k8": int(ci.workspace_bytes), "gmres_multi30_k8": int(gi.workspace_bytes)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
