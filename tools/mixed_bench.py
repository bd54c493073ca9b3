#!/usr/bin/env python3
"""Mixed-precision storage against pure storage on the same structure (include/bsm_rocm.h: BSM_F64_F32, BSM_C128_C64).

For each operator three handles are built from DEVICE blocks (device-side packing, no matrix byte crosses PCIe):
pure T (fp64 / complex128), mixed (T vectors over values stored as S), pure S (fp32 / complex64).  Each is timed as
K back-to-back products between two hip events (after 30 warm-up launches; median of three batches) and reported in
us, in stored value bytes per second and in algorithmic bytes per second (bsm_stats alg_bytes: S bytes for the values,
T bytes for x and y).  Parity of the mixed product: against the CPU oracle on the ROUNDED blocks (C2, C3, BEM), or --
the 1 GB leg, whose oracle run would take minutes -- against the pure-T handle of the rounded blocks.

usage: mixed_bench.py [--reps K] [--only c2,leg,c3,bem] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bsm_amd as bsm  # noqa: E402
from _common import N, fixture_problem, oracle_mul, relerr  # noqa: E402

S = bsm.synthetic


def timed(A, x, reps):
    y = torch.full((A.size[0],), float("nan"), dtype=x.dtype, device="cuda")
    plan = bsm.MulPlan(y, A, x)
    for _ in range(30):
        plan()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            plan()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / reps)
    return sorted(ts)[1], y


def row(A, t):
    st = A.stats()
    vb = st["stored_entries"] * A.storage_dtype.itemsize
    return {"us": round(t * 1e6, 2), "stored_GBps": round(vb / t / 1e9, 1), "alg_GBps": round(st["alg_bytes"] / t / 1e9, 1),
            "value_MB": round(vb / 1e6, 1), "alg_MB": round(st["alg_bytes"] / 1e6, 1)}


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


def case(name, host_T, dev_T, dev_S, x, reps, oracle=None):
    """host_T: host problem of type T (None: no oracle); dev_T / dev_S: the same problem on device blocks of T / S"""
    Tt = np.dtype(np.complex128 if x.dtype == torch.complex128 else np.float64)
    Sd = np.dtype(np.complex64 if Tt.kind == "c" else np.float32)
    out = {}
    A = S.build(dev_T)
    t, _ = timed(A, x, reps)
    out["pure_T"] = row(A, t)
    del A
    M = S.build(dev_T, storage=Sd)
    t, ym = timed(M, x, reps)
    out["mixed"] = row(M, t)
    ymh = ym.cpu().numpy()
    del M
    # pure S: its own vectors in S
    As = S.build(dev_S)
    xs = x.to(torch.complex64 if Tt.kind == "c" else torch.float32)
    t, _ = timed(As, xs, reps)
    out["pure_S"] = row(As, t)
    del As
    if host_T is not None and oracle is not None:
        rounded = with_blocks(host_T, lambda b: np.asfortranarray(b.astype(Sd).astype(Tt)))
        ref = oracle_mul(oracle, rounded, N, x.cpu().numpy(), np.zeros(len(ymh), Tt))
        out["parity_vs_oracle_rounded"] = float(relerr(ymh, ref))
    else:  # pure T handle of the rounded blocks, built on the device from the S blocks
        R = S.build(with_blocks(dev_S, lambda b: b.to(torch.complex128 if Tt.kind == "c" else torch.float64)))
        yr = torch.zeros(R.size[0], dtype=x.dtype, device="cuda")
        bsm.mul(yr, R, x)
        torch.cuda.synchronize()
        out["parity_vs_pure_T_rounded"] = float(relerr(ymh, yr.cpu().numpy()))
        del R
    mt, mx, ms = out["pure_T"]["us"], out["mixed"]["us"], out["pure_S"]["us"]
    out["mixed_over_T"] = round(mx / mt, 3)
    out["mixed_over_S"] = round(mx / ms, 3)
    print(f"{name:10s} T {mt:9.1f} us  mixed {mx:9.1f} us  S {ms:9.1f} us   mixed/T {mx / mt:.3f}  mixed/S {mx / ms:.3f}  "
          f"stored GB/s {out['mixed']['stored_GBps']}  parity {out.get('parity_vs_oracle_rounded', out.get('parity_vs_pure_T_rounded')):.2e}",
          flush=True)
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="c2,leg,c3,bem")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oracle import load_oracle
    orc = load_oracle()
    torch.cuda.set_device(0)
    which = a.only.split(",")
    res = {"version": bsm._lib.lib().bsm_version().decode(), "reps": a.reps}
    if "c2" in which:
        h = S.config2()
        x = torch.from_numpy(h["x"]).cuda()
        res["c2"] = case("C2", h, with_blocks(h, lambda b: dev_blocks([b])[0]),
                         with_blocks(h, lambda b: dev_blocks([b.astype(np.float32)])[0]), x, a.reps, orc)
    if "leg" in which:
        kw = dict(n=2_000_000, nblocks=100_000)
        dT = S.config2(on_device=True, **kw)
        dS = S.config2(on_device=True, dtype=np.float32, **kw)
        x = dT["x"] if isinstance(dT["x"], torch.Tensor) else torch.from_numpy(dT["x"]).cuda()
        res["vbcrs_1gb"] = case("VBCRS 1GB", None, dT, dS, x, a.reps)
        del dT, dS
    if "c3" in which:
        h = S.config3()
        x = torch.from_numpy(h["x"]).cuda()
        res["c3"] = case("C3", h, with_blocks(h, lambda b: dev_blocks([b])[0]),
                         with_blocks(h, lambda b: dev_blocks([b.astype(np.float32)])[0]), x, a.reps, orc)
    if "bem" in which:
        h = bem_tiled()
        x = torch.from_numpy(np.random.default_rng(0).standard_normal(h["size"][0]).astype(np.complex128)).cuda()
        res["bem_c128"] = case("BEM c128", h, with_blocks(h, lambda b: dev_blocks([b])[0]),
                               with_blocks(h, lambda b: dev_blocks([b.astype(np.complex64)])[0]), x, a.reps, orc)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
