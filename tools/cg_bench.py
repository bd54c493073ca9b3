#!/usr/bin/env python3
"""Developer probe: CG / COCG on the device (bsm.Cg: bsm_cg_solve), in the manner of tools/gmres_bench.py.  Every solve
runs a fixed count of iterations (rtol = 0, maxiter = --iters); `reps` timed windows after one warm-up window, each window
`solves` solves in a row, host clock around calls that end in a device synchronise, native and baseline windows
alternating; [min, median, max].  Three comparisons, one JSON line per operator, build id included:
  1. K = 1: Cg against the SAME recurrences composed of torch ops around bsm.mul with .item() for the scalars -- what a
     user could do before the solver existed                                        (native_ms_per_it / torch_ms_per_it)
  2. K = 1: Cg against Gmres(30) per iteration on the same operator                                   (gmres_ms_per_it)
  3. K = 8 in one Cg against 8 solves with K = 1 on the same solver object             (k8_ms_per_it / k1x8_ms_per_it)
Operators:
  c3    SymmetricBlockMatrix, 200 000 rows, float64, generated in HBM, M = block_jacobi(A) over its diagonalindices (CG)
  bem   the reference's BEM fixture (tests/golden/symmetric_cuboid.bin, ComplexF64, complex symmetric) tiled --tiles times
        along the diagonal as tools/bem_real.py does, M = block_jacobi(A) (COCG)
Definiteness: a generated operator need not be definite.  Before anything is timed a probe solve of K = 1 runs the
count; if its column does not reach maxiter (a non-finite residual or a breakdown froze it), if its residual norm ends
at or above ||b|| (an indefinite operator: the recurrence runs, finite, and does not converge), or --shift is given, the
diagonal blocks are shifted through bsm.update_blocks, A <- A + s I, and M is built from the shifted operator.  s = --shift,
or with --shift auto (the default) 1.1 x an estimate of the spectral radius (30 power iterations on bsm.mul): the spectrum
of a real symmetric A then lies in (0.1, 2.1) x radius.  "shift" and "shift_needed" record what happened; "status" holds
the column statuses of the timed solves (1 everywhere: every column ran the whole count).
  vec_model_bytes / vec_gbs_lower_bound   the vector work of one iteration as the kernels move it -- cg_dot 2, cg_update 6
        (x, r read and written, p, q read), cg_dir 3, with M another cg_dot: 13 n s bytes per column -- over (solve time -
        products): an upper bound of its time (the host's share is in it), so a lower bound of its rate
usage: cg_bench.py [--only c3,bem] [--reps 5] [--solves 10] [--iters 60] [--tiles 200] [--shift auto|S] [--no-torch]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bsm_amd as bsm  # noqa: E402
from bsm_amd import _lib as L  # noqa: E402

S = bsm.synthetic


def stats(ts, scale=1e3, digits=4):
    ts = sorted(ts)
    return [round(ts[0] * scale, digits), round(ts[len(ts) // 2] * scale, digits), round(ts[-1] * scale, digits)]


def med(ts):
    return sorted(ts)[len(ts) // 2]


def bem_problem(tiles):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from _common import fixture_problem
    p = fixture_problem("cuboid")
    n0 = p["size"][0]

    def tile(lists):
        return [l + k * n0 for k in range(tiles) for l in lists]
    return dict(kind="symmetric", diagonals=p["diagonals"] * tiles, diagonalindices=tile(p["diagonalindices"]),
                offdiagonals=p["offdiagonals"] * tiles, rowindices=tile(p["rowindices"]), colindices=tile(p["colindices"]),
                size=(n0 * tiles, n0 * tiles))


def spectral_radius(torch, A, n, dt, its=30):
    v = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, n).astype(dt)).cuda()
    w = torch.empty_like(v)
    rho = 0.0
    for _ in range(its):
        bsm.mul(w, A, v)
        rho = (torch.linalg.vector_norm(w) / torch.linalg.vector_norm(v)).item()
        v, w = w / torch.linalg.vector_norm(w), v
    return rho


def shift_diagonal(torch, A, s):
    """A <- A + s I through update_blocks on the diagonal blocks (ids 1 .. number of diagonals)"""
    ids = list(bsm.eachdiagonalindex(A))
    new = []
    for i in ids:
        d = bsm.diagonal(A, i)
        if isinstance(d, torch.Tensor):
            new.append(d + s * torch.eye(d.shape[0], dtype=d.dtype, device=d.device))
        else:
            new.append(np.asfortranarray(np.asarray(d) + s * np.eye(d.shape[0], dtype=d.dtype)))
    bsm.update_blocks(A, new, ids=ids)
    torch.cuda.synchronize()


def torch_cg(torch, A, M, b, iters, conj):
    """the baseline: the recurrences of bsm_cg_solve, every vector operation a torch op, every scalar through .item()"""
    def form(u, v):
        return (torch.vdot(u, v) if conj else torch.dot(u, v)).item()
    x, r = torch.zeros_like(b), b.clone()
    z, q = torch.empty_like(b), torch.empty_like(b)
    if M is not None:
        bsm.mul(z, M, r)
    else:
        z = r
    p = z.clone()
    rz = form(r, z)
    rn = 0.0
    for _ in range(iters):
        bsm.mul(q, A, p)
        alpha = rz / form(p, q)
        x.add_(p, alpha=alpha)
        r.sub_(q, alpha=alpha)
        rn = torch.linalg.vector_norm(r).item()
        if M is not None:
            bsm.mul(z, M, r)
        rzn = form(r, z)
        p.mul_(rzn / rz).add_(z)
        rz = rzn
    torch.cuda.synchronize()
    return x, rn


def window(torch, fn, solves):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(solves):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / solves, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c3,bem")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--tiles", type=int, default=200)
    ap.add_argument("--shift", default="auto")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    for name in a.only.split(","):
        A = S.build(S.config3(on_device=True) if name == "c3" else bem_problem(a.tiles))
        n, dt = A.size[0], A.dtype
        cplx = dt.kind == "c"
        method = "cocg" if cplx else "cg"
        probe_b = torch.from_numpy(np.random.default_rng(0xC6).uniform(-1, 1, n).astype(dt)).cuda()
        probe = bsm.Cg(A, bsm.block_jacobi(A), method=method).solve(probe_b, rtol=0.0, maxiter=a.iters)[1]
        # frozen inside the count, or the residual did not come down: the operator is not one the method is for
        needed = probe.column_status.tolist() != [1] or not probe.residual[0] < probe.bnorm[0]
        shift = 0.0
        if a.shift != "auto":
            shift = float(a.shift)
        elif needed:
            shift = 1.1 * spectral_radius(torch, A, n, dt)
        if shift:
            shift_diagonal(torch, A, shift)
        M = bsm.block_jacobi(A)
        rng = np.random.default_rng(0xC6)
        Bh = rng.uniform(-1, 1, (8, n)) + (1j * rng.uniform(-1, 1, (8, n)) if cplx else 0)
        B = torch.from_numpy(Bh.astype(dt)).cuda().t()  # column-major n x 8
        b = B[:, 0].contiguous()
        X = torch.empty((8, n), dtype=B.dtype, device="cuda").t()
        s1, s8 = bsm.Cg(A, M, nrhs=1, method=method), bsm.Cg(A, M, nrhs=8, method=method)
        g = bsm.Gmres(A, M, restart=30)
        out = {"op": name, "build": build_id, "n": n, "dtype": dt.name, "method": method, "iterations": a.iters,
               "solves_per_window": a.solves, "windows": a.reps, "shift": round(shift, 3), "shift_needed": needed,
               "probe_status_unshifted": probe.column_status.tolist(), "probe_iterations_unshifted": int(probe.iterations),
               "probe_relative_residual_unshifted": float(probe.residual[0] / probe.bnorm[0])}

        def k1():
            return s1.solve(b, rtol=0.0, maxiter=a.iters)[1]

        def k8():
            return s8.solve(B, X=X, rtol=0.0, maxiter=a.iters)[1]

        def k1x8():
            for c in range(8):
                info = s8.solve(B[:, c:c + 1], X=X[:, c:c + 1], rtol=0.0, maxiter=a.iters)[1]
            return info

        def gm():
            return g.solve(b, rtol=0.0, maxiter=a.iters)[1]

        def tc():
            return torch_cg(torch, A, M, b, a.iters, not cplx)
        runs = {"native": k1, "gmres": gm, "k8": k8, "k1x8": k1x8}
        if not a.no_torch:
            runs["torch"] = tc
        times = {k: [] for k in runs}
        last = {}
        for r in range(a.reps + 1):  # the first round warms up; the windows alternate
            for k, fn in runs.items():
                dtm, last[k] = window(torch, fn, a.solves)
                if r:
                    times[k].append(dtm)
        i1, i8 = last["native"], last["k8"]
        out["status"] = {"k1": i1.column_status.tolist(), "k8": i8.column_status.tolist()}
        out["k1_iterations"] = int(i1.iterations)
        out["relative_residual_native"] = float(i1.residual[0] / i1.bnorm[0])
        out["relative_residual_gmres30"] = float(last["gmres"].residual / last["gmres"].bnorm)
        # the product pair q = A p, z = M r on its own, one column and eight
        y1, Y8 = torch.empty_like(b), torch.empty((8, n), dtype=B.dtype, device="cuda").t()

        def pairs(x, y, count=100):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(count):
                bsm.mul(y, A, x)
                bsm.mul(y, M, x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / count
        pairs(b, y1, 10), pairs(B, Y8, 10)
        p1, p8 = med([pairs(b, y1) for _ in range(a.reps)]), med([pairs(B, Y8) for _ in range(a.reps)])
        out["pair_us_k1"], out["pair_us_k8"] = round(p1 * 1e6, 2), round(p8 * 1e6, 2)
        for k in times:
            out[("native" if k == "native" else k) + "_ms_per_it"] = stats([t / a.iters for t in times[k]])
        nat = med(times["native"])
        out["native_outside_products"] = round(1 - a.iters * p1 / nat, 4)
        model = 13 * n * dt.itemsize
        out["vec_model_bytes_per_it_and_column"] = model
        out["vec_gbs_lower_bound_k1"] = round(a.iters * model / max(nat - a.iters * p1, 1e-9) / 1e9, 1)
        out["vec_gbs_lower_bound_k8"] = round(8 * a.iters * model / max(med(times["k8"]) - a.iters * p8, 1e-9) / 1e9, 1)
        out["speedup_over_gmres30_per_it"] = round(med(times["gmres"]) / nat, 3)
        out["speedup_k8_over_8_k1"] = round(med(times["k1x8"]) / med(times["k8"]), 3)
        if "torch" in times:
            out["relative_residual_torch"] = float(last["torch"][1] / i1.bnorm[0])
            out["speedup_over_torch"] = round(med(times["torch"]) / nat, 3)
        out["workspace_bytes_k1"], out["workspace_bytes_k8"] = int(i1.workspace_bytes), int(i8.workspace_bytes)
        out["workspace_bytes_gmres30"] = int(last["gmres"].workspace_bytes)
        print(json.dumps(out), flush=True)
        del s1, s8, g, A, M
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
