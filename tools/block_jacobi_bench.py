#!/usr/bin/env python3
"""Developer probe: building the block-Jacobi preconditioner M = sum_s E_s inv(A[I_s, I_s]) E_s^T of a symmetric
operator over its own diagonalindices -- on the device (block_jacobi: bsm_submatrices into device windows,
bsm_invert_blocks, a BlockSparseMatrix from the device tensors) against the route a user had before (submatrices to
the host, numpy.linalg.inv per block, a BlockSparseMatrix from host blocks).

Per operator (generated in HBM), `reps` repetitions after one warm-up, host clock around calls that end in a device
synchronise, [min, median, max] in ms:
  extract_ms      submatrices(A, sets, device=True)
  invert_ms       invert_blocks on freshly extracted device blocks (the extraction before it is not timed)
  build_ms        BlockSparseMatrix(inverted device blocks, sets, sets, size): analysis + device pack
  device_ms       block_jacobi(A): the three together
  refresh_ms      M.refresh(): extract, invert, update_blocks into the existing image
  host_extract_ms / host_inv_ms / host_build_ms / host_ms     the host route and its parts (`host_reps` repetitions)
One JSON line per operator, build id included; `blocks`, `order_min/max` describe the sets.
Kernel time of the inverse alone: rocprofv3 --kernel-trace --stats -- python3 tools/block_jacobi_bench.py --only c3 --legs invert
usage: block_jacobi_bench.py [--only c3,c5s] [--reps 5] [--host-reps 3] [--legs extract,invert,build,device,refresh,host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

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
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--legs", default="extract,invert,build,device,refresh,host")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]

    def timed(fn, reps, before=None):
        ts = []
        for r in range(reps + 1):  # the first one warms up
            arg = before() if before else None
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(arg) if before else fn()
            torch.cuda.synchronize()
            if r:
                ts.append(time.perf_counter() - t)
        return ts

    for name in a.only.split(","):
        A = S.build(OPS[name]())
        torch.cuda.synchronize()
        sets = A.diagonalindices
        orders = [len(s) for s in sets]
        out = {"op": name, "build": build_id, "size": list(A.size), "dtype": A.dtype.name, "blocks": len(sets),
               "order_min": min(orders), "order_max": max(orders), "block_bytes": int(sum(o * o for o in orders) * A.dtype.itemsize)}
        if "extract" in legs:
            out["extract_ms"] = stats(timed(lambda: bsm.submatrices(A, sets, device=True), a.reps))
        if "invert" in legs:
            info = []
            out["invert_ms"] = stats(timed(lambda blocks: info.append(bsm.invert_blocks(blocks)), a.reps,
                                           before=lambda: bsm.submatrices(A, sets, device=True)))
            out["singular"] = int(np.count_nonzero(info[-1]))
        if "build" in legs:
            inv = bsm.submatrices(A, sets, device=True)
            bsm.invert_blocks(inv)
            out["build_ms"] = stats(timed(lambda: bsm.BlockSparseMatrix(inv, sets, sets, A.size), a.reps))
        M = None
        if "device" in legs or "refresh" in legs:
            ts = timed(lambda: bsm.block_jacobi(A), a.reps)
            if "device" in legs:
                out["device_ms"] = stats(ts)
        if "refresh" in legs:
            M = bsm.block_jacobi(A)
            out["refresh_ms"] = stats(timed(lambda: M.refresh(), a.reps))
            out["M_device_bytes"] = M.stats()["device_bytes"]
        if "host" in legs:
            parts = {"host_extract_ms": [], "host_inv_ms": [], "host_build_ms": [], "host_ms": []}
            for r in range(a.host_reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                blocks = bsm.submatrices(A, sets)
                t1 = time.perf_counter()
                inv = [np.asfortranarray(np.linalg.inv(b)) for b in blocks]
                t2 = time.perf_counter()
                H = bsm.BlockSparseMatrix(inv, sets, sets, A.size)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                if r:
                    for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                        parts[k].append(v)
                del H
            out.update({k: stats(v) for k, v in parts.items()})
        print(json.dumps(out), flush=True)
        del A, M
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
