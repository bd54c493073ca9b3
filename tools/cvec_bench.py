#!/usr/bin/env python3
"""Complex vectors under a real operator (include/bsm_rocm.h: bsm_mul_cvec / bsm_mul_multi_cvec) against the other ways
to get the same product.  For each operator, built in float64 from DEVICE blocks (no matrix byte crosses PCIe):

    real      the real product on the handle (float64 x, y)
    cvec      the complex-vector product on the same handle (complex128 x, y): one pass over the matrix
    two_real  A * real(x) and A * imag(x) as two real products plus the recombination on the device (what the Julia
              binding's fallback did before, minus its host round trips: a lower bound of that path)
    complex   the same operator built as complex128 (imaginary parts zero), complex128 x, y

Each is timed as K back-to-back calls between two hip events (after 30 warm-up calls; median of three batches).
Several right-hand sides (C3, tiled BEM real part, 1 GB leg): x 8 complex columns against x 16 real columns on the same
handle (the same interleaved pass over 16 components) and against 8 one-column complex products.  Parity of the cvec
product: against the CPU oracle on the complex-promoted problem (C2, C3, BEM), or -- the 1 GB leg -- against the
complex handle.

usage: cvec_bench.py [--reps K] [--only c2,leg,c3,bem] [--out FILE]
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


def bem_real_tiled(K=400):
    p = fixture_problem("cuboid", dtype=np.float64, part="real")
    n0 = p["size"][0]
    tile = lambda lists: [v + k * n0 for k in range(K) for v in lists]  # noqa: E731
    return dict(kind="symmetric", diagonals=p["diagonals"] * K, diagonalindices=tile(p["diagonalindices"]),
                offdiagonals=p["offdiagonals"] * K, rowindices=tile(p["rowindices"]), colindices=tile(p["colindices"]),
                size=(n0 * K, n0 * K))


def colmajor(k, n, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((k, n), dtype=dtype, device="cuda", generator=g).t()


def case(name, host, dev, reps, oracle=None, multi=False):
    """host: host problem (None: no oracle); dev: the same problem on float64 device blocks"""
    out = {}
    A = S.build(dev)
    m, n = A.size
    xr = colmajor(1, n, torch.float64, 1)[:, 0].contiguous()
    xi = colmajor(1, n, torch.float64, 2)[:, 0].contiguous()
    xc = torch.complex(xr, xi)
    yr = torch.empty(m, dtype=torch.float64, device="cuda")
    yi = torch.empty_like(yr)
    yc = torch.empty(m, dtype=torch.complex128, device="cuda")
    pr, pi, pc = bsm.MulPlan(yr, A, xr), bsm.MulPlan(yi, A, xi), bsm.MulPlan(yc, A, xc)
    out["real_us"] = timed(pr, reps)
    out["cvec_us"] = timed(pc, reps)
    out["two_real_us"] = timed(lambda: (pr(), pi(), torch.complex(yr, yi)), reps)
    pc()
    torch.cuda.synchronize()
    ycv = yc.cpu().numpy()
    if multi:
        k = 8
        Xc = colmajor(k, n, torch.complex128, 3)
        Yc = colmajor(k, m, torch.complex128, 4)
        Xr = colmajor(2 * k, n, torch.float64, 5)
        Yr = colmajor(2 * k, m, torch.float64, 6)
        cols = [(Xc[:, j].contiguous(), Yc[:, j].contiguous()) for j in range(k)]
        plans = [bsm.MulPlan(yj, A, xj) for xj, yj in cols]
        out["x8_cvec_us"] = timed(lambda: bsm.mul(Yc, A, Xc), reps)
        out["x16_real_us"] = timed(lambda: bsm.mul(Yr, A, Xr), reps)
        out["8x_one_cvec_us"] = timed(lambda: [p() for p in plans], max(reps // 4, 3))
        out["x8_over_x16"] = round(out["x8_cvec_us"] / out["x16_real_us"], 3)
        out["x8_over_8x_one"] = round(out["x8_cvec_us"] / out["8x_one_cvec_us"], 3)
        del Xc, Yc, Xr, Yr, cols, plans
    del A, pr, pi, pc
    torch.cuda.empty_cache()
    Ac = S.build(with_blocks(dev, lambda b: b.to(torch.complex128)))
    yc2 = torch.empty(m, dtype=torch.complex128, device="cuda")
    out["complex_us"] = timed(bsm.MulPlan(yc2, Ac, xc), reps)
    if host is not None and oracle is not None:
        ref = oracle_mul(oracle, with_blocks(host, lambda b: np.asfortranarray(b.astype(np.complex128))), N,
                         xc.cpu().numpy(), np.zeros(m, np.complex128))
        out["parity_vs_oracle"] = float(relerr(ycv, ref))
    else:
        bsm.mul(yc2, Ac, xc)
        torch.cuda.synchronize()
        out["parity_vs_complex_handle"] = float(relerr(ycv, yc2.cpu().numpy()))
    del Ac
    torch.cuda.empty_cache()
    out["cvec_over_real"] = round(out["cvec_us"] / out["real_us"], 3)
    out["cvec_over_two_real"] = round(out["cvec_us"] / out["two_real_us"], 3)
    out["cvec_over_complex"] = round(out["cvec_us"] / out["complex_us"], 3)
    print(f"{name:10s} real {out['real_us']:9.1f}  cvec {out['cvec_us']:9.1f}  two real {out['two_real_us']:9.1f}  "
          f"complex {out['complex_us']:9.1f} us   cvec/real {out['cvec_over_real']:.3f}  cvec/two {out['cvec_over_two_real']:.3f}"
          + (f"   x8 {out['x8_cvec_us']:.1f}  x16 real {out['x16_real_us']:.1f}  8 x one {out['8x_one_cvec_us']:.1f} us"
             if multi else ""), flush=True)
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
        res["c2"] = case("C2", h, with_blocks(h, lambda b: dev_blocks([b])[0]), a.reps, orc)
    if "leg" in which:
        d = S.config2(on_device=True, n=2_000_000, nblocks=100_000)
        res["vbcrs_1gb"] = case("VBCRS 1GB", None, d, a.reps, multi=True)
        del d
    if "c3" in which:
        h = S.config3()
        res["c3"] = case("C3", h, with_blocks(h, lambda b: dev_blocks([b])[0]), a.reps, orc, multi=True)
    if "bem" in which:
        h = bem_real_tiled()
        res["bem_real"] = case("BEM real", h, with_blocks(h, lambda b: dev_blocks([b])[0]), a.reps, orc, multi=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
