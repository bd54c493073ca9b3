#!/usr/bin/env python3
"""Developer probe: do two builds of the library give the same BITS on the lockstep solvers and the Gram-Schmidt pass?
One invocation runs a fixed list of solves with the library named by BSM_LIB (default: the tree's) in a fresh process and
writes a JSON of digests; --diff compares two such files.  For changes that move the solver kernels' code about without
reordering a sum: every digest must then be equal.

The operators are those of tests/_lockstep.py::grid_case: block diagonal VBCRS, with M the block-Jacobi preconditioner over
half_sets.  Their products add every row's terms in one wave in a fixed order (stats()["exclusive"] == 1, asserted here for
every A and M before anything is solved), so two runs of one build agree bit for bit and a difference between two builds
is a difference of the solver kernels.

  cases   the G = 2 and G = 3 rows of rows_of(dtype) in all four types and one G = 65 row (float32, float64); K = 1, 3, 16;
          cg, cocg (complex types), bicgstab, gmres_multi (restart 5: a restart happens) and Gmres (one column); each
          without M, with M, and from an initial guess X0; maxiter = 12, rtol = 1e-30 (every column runs the whole count
          unless it freezes).  Then krylov_orth, k = 5, n = 2051 in all four types with w one element past a 16-byte
          boundary: V aligned (the element-wise kernels) and V as far off as w (16-byte groups with a guarded head), and
          both aligned.
  digest  sha256 of X, of the history, and the info / column fields (the workspace address left out)

--time-orth: krylov_orth alone, float64, n = 200 000, k = 30, by the window protocol of tools/cg_bench.py (`reps` timed
windows after a warm-up window, each `calls` passes in a row, host clock around a device synchronise) -> one JSON line.

usage: lockstep_ab.py OUT.json | --diff A.json B.json | --time-orth [--reps 5] [--calls 200]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

MAXITER, RTOL, RESTART = 12, 1e-30, 5
TYPES = [np.complex128, np.float64, np.float32, np.complex64]
BIG = {"float32": 131073, "float64": 65537}  # one G = 65 row each


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def diff(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    only = sorted(set(a["cases"]) ^ set(b["cases"]))
    bad = sorted(k for k in set(a["cases"]) & set(b["cases"]) if a["cases"][k] != b["cases"][k])
    for k in bad:
        print("differs:", k, {f: (a["cases"][k][f], b["cases"][k][f]) for f in a["cases"][k]
                               if a["cases"][k][f] != b["cases"][k].get(f) and f not in ("x", "history")})
    for k in only:
        print("on one side only:", k)
    print(json.dumps({"a": a["lib"], "b": b["lib"], "build_a": a["build"], "build_b": b["build"], "cases": len(a["cases"]),
                      "equal": len(set(a["cases"]) & set(b["cases"])) - len(bad), "different": len(bad), "one_sided": len(only)}))
    return 1 if bad or only else 0


def time_orth(reps, calls):
    import torch
    import bsm_amd as bsm
    from bsm_amd import _lib as L
    from cg_bench import stats, window
    n, k, dt = 200_000, 30, np.float64
    rng = np.random.default_rng(0x0A7)
    V = torch.from_numpy(rng.uniform(-1, 1, (k, n)).astype(dt)).cuda().t()
    w0 = torch.from_numpy(rng.uniform(-1, 1, n).astype(dt)).cuda()
    w, hsum, nrm = w0.clone(), torch.zeros(k, dtype=w0.dtype, device="cuda"), torch.zeros(1, dtype=w0.dtype, device="cuda")
    work = torch.empty(bsm.krylov_orth_work(dt, n, k) + 16, dtype=torch.uint8, device="cuda")
    times = []
    for r in range(reps + 1):  # the first window warms up
        w.copy_(w0)
        t, _ = window(torch, lambda: bsm.krylov_orth(V, w, k, hsum, nrm, work), calls)
        if r:
            times.append(t)
    print(json.dumps({"probe": "krylov_orth", "build": L.lib().bsm_version().decode().split()[-1], "lib": L.LIB_PATH, "n": n, "k": k,
                      "dtype": "float64", "windows": reps, "calls_per_window": calls, "us_per_pass": stats(times, 1e6, 3)}), flush=True)
    return 0


def solve_cases(torch, bsm, out):
    from _cg import MAX_RHS
    from _jacobi import uniform
    from _lockstep import COLUMNS, block_solve, grid_case, half_sets, rows_of

    def run(key, S, B, X0, one_column=False):
        Bd = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().t()
        if one_column:
            Bd = Bd[:, 0].contiguous()
        kw = {}
        if X0 is not None:
            X0d = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda().t()
            kw["x0" if one_column else "X0"] = X0d[:, 0].contiguous() if one_column else X0d
        X, info = S.solve(Bd, rtol=RTOL, maxiter=MAXITER, **kw)
        torch.cuda.synchronize()
        rec = {"x": sha(X.cpu().numpy()), "history": sha(info.history), "status": int(info.status), "iterations": int(info.iterations),
               "a_products": int(info.a_products), "m_products": int(info.m_products), "workspace_bytes": int(info.workspace_bytes)}
        if one_column:
            rec.update(cycles=int(info.cycles), residual=float(info.residual).hex(), bnorm=float(info.bnorm).hex())
        else:
            rec.update(columns_converged=int(info.columns_converged), column_status=info.column_status.tolist(),
                       column_iterations=info.column_iterations.tolist(), residual=[float(v).hex() for v in info.residual],
                       bnorm=[float(v).hex() for v in info.bnorm])
        out[key] = rec

    for dt in TYPES:
        name = np.dtype(dt).name
        sizes = [n for n, G in rows_of(dt) if G in (2, 3)] + ([BIG[name]] if name in BIG else [])
        methods = ["cg"] + (["cocg"] if np.dtype(dt).kind == "c" else []) + ["bicgstab", "gmres_multi", "gmres"]
        for n in sizes:
            for method in methods:
                prob, Dop, B = grid_case("bicgstab" if method.startswith("gmres") else method, n, dt)
                A = bsm.synthetic.build(prob)
                M = bsm.block_jacobi(A, half_sets(n))
                assert A.stats()["exclusive"] == 1 and M.stats()["exclusive"] == 1, ("products not reproducible", method, name, n)
                sol = block_solve(Dop, B)
                X0 = np.asfortranarray((sol + 1e-2 * np.max(np.abs(sol)) * uniform(np.random.default_rng(8900 + n), sol.shape, dt)).astype(dt))
                for var, m, x0 in (("plain", None, None), ("M", M, None), ("X0", None, X0)):
                    if method == "gmres":
                        run(f"gmres {name} n={n} {var}", bsm.Gmres(A, m, restart=RESTART), B[:, :1], None if x0 is None else x0[:, :1], True)
                        continue
                    if method == "gmres_multi":
                        S = bsm.GmresMulti(A, m, nrhs=MAX_RHS, restart=RESTART)
                    elif method == "bicgstab":
                        S = bsm.BiCgStab(A, m, nrhs=MAX_RHS)
                    else:
                        S = bsm.Cg(A, m, nrhs=MAX_RHS, method=method)
                    for k in COLUMNS:
                        run(f"{method} {name} n={n} K={k} {var}", S, np.asfortranarray(B[:, :k]), None if x0 is None else np.asfortranarray(x0[:, :k]))
                del A, M


def orth_cases(torch, bsm, out):
    n, k = 2051, 5
    for dt in TYPES:
        name = np.dtype(dt).name
        ve = 16 // np.dtype(dt).itemsize
        ld = (n + 1 + ve - 1) // ve * ve
        rng = np.random.default_rng(0x0A8)

        def rand(shape):
            a = rng.uniform(-1, 1, shape)
            return (a + 1j * rng.uniform(-1, 1, shape) if np.dtype(dt).kind == "c" else a).astype(dt)
        Vh, wh = rand((k, n)), rand(n)
        for tag, voff, woff in (("aligned", 0, 0), ("w off, V aligned", 0, 1), ("w and V off", 1, 1)):
            vbuf = torch.zeros(k * ld + 1, dtype=torch.from_numpy(Vh).dtype, device="cuda")
            V = vbuf[voff:voff + k * ld].view(k, ld).t()[:n]
            V.copy_(torch.from_numpy(Vh).cuda().t())
            wbuf = torch.zeros(n + 2, dtype=vbuf.dtype, device="cuda")
            w = wbuf[woff:woff + n]
            w.copy_(torch.from_numpy(wh).cuda())
            assert vbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
            hsum = torch.zeros(k, dtype=vbuf.dtype, device="cuda")
            nrm = torch.zeros(1, dtype=torch.from_numpy(np.zeros(1, dt).real).dtype, device="cuda")
            bsm.krylov_orth(V, w, k, hsum, nrm)
            torch.cuda.synchronize()
            out[f"krylov_orth {name} n={n} k={k} {tag}"] = {"x": sha(wbuf.cpu().numpy()), "history": sha(hsum.cpu().numpy()),
                                                           "nrm": float(nrm.cpu().numpy()[0]).hex()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--diff", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--time-orth", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    if a.diff:
        return diff(*a.diff)
    if a.time_orth:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        return time_orth(a.reps, a.calls)
    if not a.out:
        ap.error("OUT.json, --diff or --time-orth")
    import torch
    import bsm_amd as bsm
    from bsm_amd import _lib as L
    t = time.perf_counter()
    cases = {}
    solve_cases(torch, bsm, cases)
    orth_cases(torch, bsm, cases)
    json.dump({"lib": L.LIB_PATH, "build": L.lib().bsm_version().decode().split()[-1], "cases": cases}, open(a.out, "w"), indent=0)
    print(f"{len(cases)} cases in {time.perf_counter() - t:.1f} s -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
