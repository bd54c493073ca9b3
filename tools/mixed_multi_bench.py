#!/usr/bin/env python3
"""Several right-hand sides on mixed-precision handles (BSM_F64_F32, BSM_C128_C64): the interleaved pass over the
single-precision image against the ways to get the same K columns.  For each operator, built from DEVICE blocks:

    mixed      A @ X on the mixed handle, K columns in one bsm_mul_multi: the pass at EVERY width (the tool sets
               BSM_IL_MIXED_MIN_COLS=2 unless the caller set it -- the library's threshold comes from this table)
    K x one    K one-column products on the same handle (what bsm_mul_multi did before the pass existed)
    pure       A @ X on the pure double-precision handle of the ROUNDED blocks
    il0        (child process, BSM_MULTI_IL=0) A @ X on the mixed handle with the pass switched off: the in-build
               cross-check of `K x one`

Each is timed as `reps` back-to-back calls between two device events (after 30 warm-up calls; median of three
batches), K in 2, 3, 4, 5, 8, 16, and the passes every call added to bsm_value_passes are recorded beside its time.
Parity: the K = 8 mixed product against the pure handle's one-column products, worst column.

usage: mixed_multi_bench.py [--reps R] [--only c2,leg,c3,bem] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("BSM_IL_MIXED_MIN_COLS", "2")  # (read once, at the library's first multi-column product)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bsm_amd as bsm  # noqa: E402
from _common import fixture_problem, relerr  # noqa: E402

S = bsm.synthetic
KS = (2, 3, 4, 5, 8, 16)


def timed(fn, reps):
    for _ in range(30):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / reps)
    return round(sorted(ts)[1] * 1e6, 2)


def dev_blocks(blocks):
    return [torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t() for b in blocks]


def with_blocks(p, f):
    q = dict(p)
    for k in ("blocks", "diagonals", "offdiagonals"):
        if k in p:
            q[k] = [f(b) for b in p[k]]
    return q


def bem_tiled(K=400):
    p = fixture_problem("cuboid")
    n0 = p["size"][0]
    tile = lambda lists: [v + k * n0 for k in range(K) for v in lists]  # noqa: E731
    return dict(kind="symmetric", diagonals=p["diagonals"] * K, diagonalindices=tile(p["diagonalindices"]),
                offdiagonals=p["offdiagonals"] * K, rowindices=tile(p["rowindices"]), colindices=tile(p["colindices"]),
                size=(n0 * K, n0 * K))


def colmajor(k, n, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((k, n), dtype=dtype, device="cuda", generator=g).t()


def passes(A, fn):
    before = A.value_passes()
    fn()
    return A.value_passes() - before


def case(name, dev, cplx, reps, ops, il0):
    """dev: the problem on device blocks of T.  il0: this is the BSM_MULTI_IL=0 child -- the mixed A @ X only"""
    tT, tS = (torch.complex128, torch.complex64) if cplx else (torch.float64, torch.float32)
    Sd = np.complex64 if cplx else np.float32
    M = S.build(dev, storage=Sd)
    R = None if il0 else S.build(with_blocks(dev, lambda b: b.to(tS).to(tT)))  # pure T of the rounded blocks
    out = {}
    for opname in ops:
        wrap = (lambda A: A) if opname == "N" else bsm.transpose
        m, n = M.size if opname == "N" else M.size[::-1]
        rows = {}
        for k in KS:
            X, Y = colmajor(k, n, tT, 3 + k), colmajor(k, m, tT, 40 + k)
            r = {}
            mixed = lambda: bsm.mul(Y, wrap(M), X)  # noqa: E731
            r["mixed_passes"] = passes(M, mixed)
            r["mixed_us"] = timed(mixed, reps)
            if not il0:
                plans = [bsm.MulPlan(Y[:, j].contiguous(), wrap(M), X[:, j].contiguous()) for j in range(k)]
                r["k_one_us"] = timed(lambda: [p() for p in plans], reps)
                pure = lambda: bsm.mul(Y, wrap(R), X)  # noqa: E731
                r["pure_passes"] = passes(R, pure)
                r["pure_us"] = timed(pure, reps)
                r["mixed_over_k_one"] = round(r["mixed_us"] / r["k_one_us"], 3)
                r["mixed_over_pure"] = round(r["mixed_us"] / r["pure_us"], 3)
                if k == 8:  # parity: every column against the pure handle's one-column product
                    mixed()
                    torch.cuda.synchronize()
                    worst = 0.0
                    for j in range(k):
                        y1 = torch.zeros(m, dtype=tT, device="cuda")
                        bsm.mul(y1, wrap(R), X[:, j].contiguous())
                        torch.cuda.synchronize()
                        worst = max(worst, relerr(Y[:, j].cpu().numpy(), y1.cpu().numpy()))
                    r["parity_vs_pure_rounded"] = float(worst)
            rows[str(k)] = r
            print(f"{name:10s} op {opname} x {k:2d}  mixed {r['mixed_us']:9.1f} us ({r['mixed_passes']} passes)"
                  + ("" if il0 else f"  {k} x one {r['k_one_us']:9.1f}  pure {r['pure_us']:9.1f} ({r['pure_passes']} passes)"
                     f"  mixed/one {r['mixed_over_k_one']:.3f}  mixed/pure {r['mixed_over_pure']:.3f}"), flush=True)
            del X, Y
        out[opname] = rows
    del M, R
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="c2,leg,c3,bem")
    ap.add_argument("--out", default=None)
    ap.add_argument("--il0-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    il0 = a.il0_child
    if il0:
        assert os.environ.get("BSM_MULTI_IL") == "0"
    torch.cuda.set_device(0)
    which = a.only.split(",")
    res = {"version": bsm._lib.lib().bsm_version().decode(), "reps": a.reps,
           "BSM_IL_MIXED_MIN_COLS": os.environ["BSM_IL_MIXED_MIN_COLS"]}
    if "c2" in which:
        h = S.config2()
        res["c2"] = case("C2", with_blocks(h, lambda b: dev_blocks([b])[0]), False, a.reps, ("N",), il0)
    if "leg" in which:
        d = S.config2(on_device=True, n=2_000_000, nblocks=100_000)
        res["vbcrs_1gb"] = case("VBCRS 1GB", d, False, a.reps, ("N", "T"), il0)
        del d
    if "c3" in which:
        h = S.config3()
        res["c3"] = case("C3", with_blocks(h, lambda b: dev_blocks([b])[0]), False, a.reps, ("N",), il0)
    if "bem" in which:
        h = bem_tiled()
        res["bem_c128"] = case("BEM c128", with_blocks(h, lambda b: dev_blocks([b])[0]), True, a.reps, ("N",), il0)
    if not il0:  # the same legs with the pass switched off, in a process of its own (the switch is read once)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--il0-child", "--reps", str(a.reps), "--only", a.only],
                           env=dict(os.environ, BSM_MULTI_IL="0"), stdout=subprocess.PIPE, timeout=1500)
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
        if r.returncode == 0 and lines:
            res["il0"] = {k: v for k, v in json.loads(lines[-1]).items() if isinstance(v, dict)}
            for leg, ops in res["il0"].items():
                for op, rows in ops.items():
                    for k, r0 in rows.items():
                        print(f"{leg:10s} op {op} x {int(k):2d}  BSM_MULTI_IL=0 {r0['mixed_us']:9.1f} us ({r0['mixed_passes']} passes)")
        else:
            res["il0"] = {"failed": r.returncode}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
