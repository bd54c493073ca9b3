#!/usr/bin/env python3
"""Developer probe: BiCGSTAB on the device (bsm.BiCgStab: bsm_bicgstab_solve), in the manner of tools/cg_bench.py, whose
window protocol and helpers it uses.  Every solve runs a fixed count of iterations (rtol = 0, maxiter = --iters); `reps`
timed windows after one warm-up window, each window `solves` solves in a row, host clock around calls that end in a device
synchronise, native and baseline windows alternating; [min, median, max].  One JSON line per operator, build id included:
  1. K = 1: BiCgStab against the SAME recurrences composed of torch ops around bsm.mul with .item() for the scalars
                                                                                    (native_ms_per_it / torch_ms_per_it)
  2. K = 1: BiCgStab against Gmres(30) on the same operator and M, per iteration and per A product (BiCGSTAB does two per
     iteration), and the workspaces                                                                   (gmres_ms_per_it)
  3. K = 8 in one BiCgStab against 8 solves with K = 1 on the same solver object    (k8_ms_per_it / k1x8_ms_per_it), beside
     the bare product pairs A x, M x at K = 1 and K = 8 (an iteration holds two pairs)
  4. the share of a solve outside the products, and the lower-bound rate of the vector kernels
Operators:
  c2    VariableBlockCompressedRowStorage, config2 (100 000 rows, float64) generated in HBM, no preconditioner.  As
        generated it is singular (5000 blocks leave block rows empty) and has no diagonal blocks -- its row and column
        segments are cut independently --, so the method breaks down on it; the tool adds one block s I per row segment
        (overlapping blocks of a VBCRS add up), s = --shift or 1.1 x the estimated spectral radius: A + s I
  c3    a C3-shaped BlockSparseMatrix: config3's band (3125 segments of 64, half band 8) with every block on BOTH sides of
        the diagonal its own draw (nonsymmetric), generated in HBM, diagonal blocks shifted by --shift (auto: 1.1 x the
        spectral radius estimated by 30 power iterations) so that the method converges, M = block_jacobi over the segments
  bem   the reference's BEM fixture (tests/golden/symmetric_cuboid.bin, ComplexF64) tiled --tiles times along the
        diagonal, shifted like cg_bench.py's, M = block_jacobi(A)
  vec_model_bytes / vec_gbs_lower_bound   the vector work of one iteration as the kernels move it -- bicg_dot 2, bicg_half 6
        (x, r read and written, phat, v read), bicg_dot 2, bicg_update 7 (x, r read and written, shat, t, rhat read; 6
        without M, where shat is r), bicg_dir 4: 21 n s bytes per column with M, 20 without -- over (solve time -
        products): an upper bound of its time (the host's share is in it), so a lower bound of its rate
usage: bicgstab_bench.py [--only c2,c3,bem] [--reps 5] [--solves 10] [--iters 60] [--tiles 200] [--shift auto|S] [--no-torch]"""
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
from cg_bench import bem_problem, med, shift_diagonal, spectral_radius, stats, window  # noqa: E402

S = bsm.synthetic


def band_blocksparse(torch, shift, nseg=3125, bs=64, halfband=8, seed=0xB5A3):
    """the C3-shaped nonsymmetric BlockSparseMatrix -> (A, sets, shift used): blocks 0 .. nseg - 1 are the diagonal ones,
    then (I, J) and (J, I) for J = I - 1 .. I - halfband, each its own draw of the config stream"""
    idx = [np.arange(i * bs + 1, (i + 1) * bs + 1, dtype=np.int64) for i in range(nseg)]
    ri, ci = list(idx), list(idx)
    for i in range(nseg):
        for k in range(1, halfband + 1):
            if i - k >= 0:
                ri += [idx[i], idx[i - k]]
                ci += [idx[i - k], idx[i]]
    nb = len(ri)
    blocks = S.device_blocks(seed, np.arange(nb), np.full(nb, bs), np.full(nb, bs), np.float64)
    n = nseg * bs
    if shift is None:
        A0 = bsm.BlockSparseMatrix(blocks, ri, ci, (n, n))
        shift = 1.1 * spectral_radius(torch, A0, n, np.dtype(np.float64))
        del A0
    for d in blocks[:nseg]:
        d.diagonal().add_(shift)
    A = bsm.BlockSparseMatrix(blocks, ri, ci, (n, n))
    torch.cuda.synchronize()
    return A, idx, shift


def shifted_c2(torch, shift):
    """config2 plus one block s I on every row segment -> (A, shift used)"""
    p = S.config2(on_device=True)
    n = p["size"][0]
    if shift is None:
        A0 = S.build(p)
        shift = 1.1 * spectral_radius(torch, A0, n, np.dtype(np.float64))
        del A0
    rstart, rsz = S.config2_row_segments(n)
    eyes = [(shift * torch.eye(int(m), dtype=torch.float64, device="cuda")).t() for m in rsz]  # (.t(): column-major strides)
    starts = np.asarray(rstart, dtype=np.int64) + 1
    A = bsm.VariableBlockCompressedRowStorage(list(p["blocks"]) + eyes, np.concatenate([p["rowstart"], starts]),
                                              np.concatenate([p["colstart"], starts]), p["size"])
    torch.cuda.synchronize()
    return A, shift


def torch_bicgstab(torch, A, M, b, iters):
    """the baseline: the recurrences of bsm_bicgstab_solve, every vector operation a torch op, every scalar through .item()"""
    x, r = torch.zeros_like(b), b.clone()
    rhat, p = r.clone(), r.clone()
    v, t, z = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
    rho = torch.vdot(rhat, r).item()
    rn = 0.0
    for _ in range(iters):
        phat = p
        if M is not None:
            bsm.mul(z, M, p)
            phat = z
        bsm.mul(v, A, phat)
        alpha = rho / torch.vdot(rhat, v).item()
        x.add_(phat, alpha=alpha)
        r.sub_(v, alpha=alpha)
        torch.linalg.vector_norm(r).item()  # sn: the solver decides on it
        shat = r
        if M is not None:
            bsm.mul(z, M, r)
            shat = z
        bsm.mul(t, A, shat)
        omega = torch.vdot(t, r).item() / torch.vdot(t, t).item()
        x.add_(shat, alpha=omega)
        r.sub_(t, alpha=omega)
        rn = torch.linalg.vector_norm(r).item()
        rhon = torch.vdot(rhat, r).item()
        beta = (rhon / rho) * (alpha / omega)
        p.sub_(v, alpha=omega).mul_(beta).add_(r)
        rho = rhon
    torch.cuda.synchronize()
    return x, rn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c2,c3,bem")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solves", type=int, default=10)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--tiles", type=int, default=200)
    ap.add_argument("--shift", default="auto")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    fixed = None if a.shift == "auto" else float(a.shift)
    for name in a.only.split(","):
        shift, sets = 0.0, None
        if name == "c2":
            (A, shift), M = shifted_c2(torch, fixed), None
        elif name == "c3":
            A, sets, shift = band_blocksparse(torch, fixed)
            M = bsm.block_jacobi(A, sets)
        else:
            A = S.build(bem_problem(a.tiles))
            shift = 1.1 * spectral_radius(torch, A, A.size[0], A.dtype) if fixed is None else fixed
            shift_diagonal(torch, A, shift)
            M = bsm.block_jacobi(A)
        n, dt = A.size[0], A.dtype
        cplx = dt.kind == "c"
        rng = np.random.default_rng(0xB1C6)
        Bh = rng.uniform(-1, 1, (8, n)) + (1j * rng.uniform(-1, 1, (8, n)) if cplx else 0)
        B = torch.from_numpy(Bh.astype(dt)).cuda().t()  # column-major n x 8
        b = B[:, 0].contiguous()
        X = torch.empty((8, n), dtype=B.dtype, device="cuda").t()
        s1, s8 = bsm.BiCgStab(A, M, nrhs=1), bsm.BiCgStab(A, M, nrhs=8)
        g = bsm.Gmres(A, M, restart=30)
        out = {"op": name, "build": build_id, "n": n, "dtype": dt.name, "kind": type(A).__name__, "preconditioner": M is not None,
               "iterations": a.iters, "solves_per_window": a.solves, "windows": a.reps, "shift": round(shift, 3)}

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
            return torch_bicgstab(torch, A, M, b, a.iters)
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
        # the product pair A x, M x on its own, one column and eight (an iteration holds two pairs)
        y1, Y8 = torch.empty_like(b), torch.empty((8, n), dtype=B.dtype, device="cuda").t()

        def pairs(x, y, count=100):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(count):
                bsm.mul(y, A, x)
                if M is not None:
                    bsm.mul(y, M, x)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) / count
        pairs(b, y1, 10), pairs(B, Y8, 10)
        p1, p8 = med([pairs(b, y1) for _ in range(a.reps)]), med([pairs(B, Y8) for _ in range(a.reps)])
        out["pair_us_k1"], out["pair_us_k8"] = round(p1 * 1e6, 2), round(p8 * 1e6, 2)
        for k in times:
            out[k + "_ms_per_it"] = stats([t / a.iters for t in times[k]])
        nat, k8t = med(times["native"]), med(times["k8"])
        out["native_outside_products"] = round(1 - 2 * a.iters * p1 / nat, 4)
        out["k8_outside_products"] = round(1 - 2 * a.iters * p8 / k8t, 4)
        model = (21 if M is not None else 20) * n * dt.itemsize
        out["vec_model_bytes_per_it_and_column"] = model
        out["vec_gbs_lower_bound_k1"] = round(a.iters * model / max(nat - 2 * a.iters * p1, 1e-9) / 1e9, 1)
        out["vec_gbs_lower_bound_k8"] = round(8 * a.iters * model / max(k8t - 2 * a.iters * p8, 1e-9) / 1e9, 1)
        out["gmres30_over_native_per_it"] = round(med(times["gmres"]) / nat, 3)
        out["gmres30_over_native_per_a_product"] = round(2 * med(times["gmres"]) / nat, 3)
        out["speedup_k8_over_8_k1"] = round(med(times["k1x8"]) / k8t, 3)
        out["k8_in_k1_iterations"] = round(k8t / nat, 3)
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
