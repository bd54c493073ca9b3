#!/usr/bin/env python3
"""Developer probe: the spectral block-Jacobi preconditioner M = sum_s E_s |A[I_s, I_s]|^-1 E_s^T of a symmetric operator
over its own diagonalindices on the device (block_jacobi(kind="abs"): bsm_submatrices into device windows, bsm_eigh_blocks,
bsm_spectral_blocks, a BlockSparseMatrix from the device tensors) and its two new steps alone, beside the explicit inverse
(kind="inverse": bsm_invert_blocks) as the yardstick.  No threshold rests on these times.

Per operator (generated in HBM), `reps` repetitions after one warm-up, host clock around calls that end in a device
synchronise, [min, median, max] in ms:
  eigh_ms         eigh_blocks on freshly extracted device blocks (the extraction before it is not timed)
  spectral_ms     spectral_blocks(V, w, "absinv") into fresh blocks
  abs_ms          block_jacobi(A, kind="abs"): extract, decompose, put together, build
  inverse_ms      block_jacobi(A): the explicit inverse
  refresh_ms      M.refresh() of the kind="abs" handle
One JSON line per operator, build id included; `blocks`, `order_min/max` describe the sets, `sweeps_max` the decomposition.
Cases: c3 (3125 diagonal blocks of 64 x 64: LDS-resident in float64) and c5s (a C5 slice, blocks of order 16 .. 256: both
regimes in one call).
usage: eigh_blocks_bench.py [--only c3,c5s] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsm_amd as bsm  # noqa: E402
from bsm_amd import _lib as L  # noqa: E402

S = bsm.synthetic
OPS = {"c3": lambda: S.config3(on_device=True), "c5s": lambda: S.config5(n=625_000, on_device=True)}


def stats(ts):
    ts = sorted(ts)
    return [round(ts[0] * 1e3, 3), round(ts[len(ts) // 2] * 1e3, 3), round(ts[-1] * 1e3, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c3,c5s")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]

    def timed(fn, before=None):
        ts = []
        for r in range(a.reps + 1):  # the first one warms up
            arg = before() if before else None
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(arg) if before else fn()
            torch.cuda.synchronize()
            if r:
                ts.append(time.perf_counter() - t)
        return ts

    for name in a.only.split(","):
        A = OPS[name]()
        sets = A.diagonalindices
        orders = [len(s) for s in sets]

        def decomposed():
            blocks = bsm.submatrices(A, sets, device=True)
            w, info, sweeps = bsm.eigh_blocks(blocks, sweeps=True)
            assert not info.any()
            return blocks, w, sweeps

        out = {"op": name, "build": build_id, "blocks": len(sets), "order_min": min(orders), "order_max": max(orders),
               "sweeps_max": int(decomposed()[2].max())}
        out["eigh_ms"] = stats(timed(lambda blocks: bsm.eigh_blocks(blocks), before=lambda: bsm.submatrices(A, sets, device=True)))
        out["spectral_ms"] = stats(timed(lambda d: bsm.spectral_blocks(d[0], d[1], "absinv"), before=decomposed))
        out["abs_ms"] = stats(timed(lambda: bsm.block_jacobi(A, kind="abs")))
        out["inverse_ms"] = stats(timed(lambda: bsm.block_jacobi(A)))
        M = bsm.block_jacobi(A, kind="abs")
        out["refresh_ms"] = stats(timed(M.refresh))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
