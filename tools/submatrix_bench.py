#!/usr/bin/env python3
"""Developer probe: reading entries out of the packed image (bsm_diag / bsm_submatrices) against the two routes that
existed before -- the COO export (bsm_rowcolvals into device arrays: reads every value byte, writes 24-32 B per entry)
and unit vectors through bsm_mul_multi (one pass over the image per 16 real / 8 complex columns).

Per operator (those of tools/update_bench.py, generated in HBM), `reps` repetitions after one warm-up, host clock
around calls that end in a device synchronise (both entries and the export are synchronous), min / median / max in ms:
  diag_ms        bsm_diag into a device vector
  blocks_ms      (symmetric operators) every diagonal block in ONE bsm_submatrices call over the operator's own
                 diagonalindices, device windows carved out of one buffer, pointer arrays built once
  column_ms      one column A[:, j], j = ncols / 2
  window_ms      the dense A[I, I] of W consecutive indices from n / 3 on (W = 4096); window_added_GBps = non-zero
                 entries of the result * element bytes / time (a lower bound of the added bytes: an entry that sums to
                 zero is not counted), beside the memory-side atomic rate of about 1300 GB/s
  export_ms      bsm_rowcolvals into device arrays allocated once
  pass_ms        one 16-column pass of unit vectors through bsm_mul_multi, device vectors; the product route of a
                 request with nj columns is ceil(nj / 16) of them: route_* = passes * median pass_ms (extrapolated)
One JSON line per operator, build id included.
Kernel time (the calls above also allocate, upload their maps and synchronise): run one leg under
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python3 tools/submatrix_bench.py --only c3 --legs window
and read extract_kernel from the stats file.
usage: submatrix_bench.py [--only c2,c2_1gb,c3,c5s] [--reps 5] [--window 4096] [--legs diag,blocks,column,window,export,pass]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsm_amd as bsm  # noqa: E402
from bsm_amd import _lib as L  # noqa: E402

S = bsm.synthetic
OPS = {"c2": lambda: S.config2(on_device=True), "c2_1gb": lambda: S.config2(n=2_000_000, nblocks=100_000, on_device=True),
       "c3": lambda: S.config3(on_device=True), "c5s": lambda: S.config5(n=625_000, on_device=True)}
I64 = C.POINTER(C.c_int64)


def stats(ts):
    ts = sorted(ts)
    return [round(ts[0] * 1e3, 4), round(ts[len(ts) // 2] * 1e3, 4), round(ts[-1] * 1e3, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c2,c2_1gb,c3,c5s")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--legs", default="diag,blocks,column,window,export,pass")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    import torch
    build_id = L.lib().bsm_version().decode().split()[-1]
    for name in a.only.split(","):
        p = OPS[name]()
        A = S.build(p)
        torch.cuda.synchronize()
        m, n = A.size
        dt, es = A.dtype, A.dtype.itemsize
        tdt = torch.from_numpy(np.zeros(1, dtype=dt)).dtype
        st = A.stats()
        stream = torch.cuda.current_stream().cuda_stream

        def timed(fn):
            fn()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            return ts

        def request(rowsets, colsets):
            """a bsm_submatrices call with everything marshalled once -> (callable, the buffer the windows live in)"""
            rs = [np.ascontiguousarray(r, dtype=np.int64) for r in rowsets]
            cs = [np.ascontiguousarray(c, dtype=np.int64) for c in colsets]
            k = len(rs)
            ni, nj = np.array([len(r) for r in rs], dtype=np.int64), np.array([len(c) for c in cs], dtype=np.int64)
            off = np.concatenate([[0], np.cumsum(ni * nj)])
            buf = torch.empty(int(off[-1]), dtype=tdt, device="cuda")
            ip, jp, op = (C.c_void_p * k)(*[r.ctypes.data for r in rs]), (C.c_void_p * k)(*[c.ctypes.data for c in cs]), \
                (C.c_void_p * k)(*[buf.data_ptr() + int(o) * es for o in off[:-1]])
            ld = np.maximum(ni, 1)
            keep = (rs, cs, ni, nj, ld, ip, jp, op)

            def call():
                L.check(L.lib().bsm_submatrices(A._h.ptr, L.BSM_OP_N, k, ip, ni.ctypes.data_as(I64), jp, nj.ctypes.data_as(I64), op,
                                                ld.ctypes.data_as(I64), L.BSM_MEM_DEVICE, stream))
            call.keep = keep
            return call, buf

        out = {"op": name, "build": build_id, "size": [m, n], "dtype": dt.name, "device_bytes": st["device_bytes"], "nnz": st["nnz"]}
        d = torch.empty(min(m, n), dtype=tdt, device="cuda")
        if "diag" in legs:
            out["diag_ms"] = stats(timed(lambda: L.check(L.lib().bsm_diag(A._h.ptr, d.data_ptr(), L.BSM_MEM_DEVICE, stream))))
        if isinstance(A, bsm.SymmetricBlockMatrix) and "blocks" in legs:
            own = [bsm.diagonalindices(A, k) for k in bsm.eachdiagonalindex(A)]
            call, buf = request(own, own)
            out["blocks_ms"] = stats(timed(call))
            out["blocks"], out["blocks_entries"] = len(own), int(buf.numel())
        if "column" in legs:
            call, _ = request([np.arange(1, m + 1)], [[n // 2]])
            out["column_ms"] = stats(timed(call))
        w = min(a.window, m, n)
        lo = min(m, n) // 3
        idx = np.arange(lo + 1, lo + w + 1)
        idx = idx[idx <= min(m, n)]
        if "window" in legs:
            call, buf = request([idx], [idx])
            ts = timed(call)
            out["window_ms"], out["window"] = stats(ts), len(idx)
            nz = int(torch.count_nonzero(buf).item())
            out["window_nonzero"] = nz
            out["window_added_GBps"] = round(nz * es / sorted(ts)[len(ts) // 2] / 1e9, 2)
        # the COO export of the same handle
        if "export" in legs:
            cnt = C.c_int64(st["nnz"])
            r = torch.empty(st["nnz"], dtype=torch.int64, device="cuda")
            c = torch.empty(st["nnz"], dtype=torch.int64, device="cuda")
            v = torch.empty(st["nnz"], dtype=tdt, device="cuda")
            out["export_ms"] = stats(timed(lambda: L.check(L.lib().bsm_rowcolvals(A._h.ptr, r.data_ptr(), c.data_ptr(), v.data_ptr(),
                                                                                   C.byref(cnt), L.BSM_MEM_DEVICE, stream))))
            del r, c, v
        # one pass of the product route: 16 unit vectors (8 for complex types) through bsm_mul_multi
        if "pass" in legs:
            kb = 8 if dt.kind == "c" else 16
            E = torch.zeros((kb, n), dtype=tdt, device="cuda").t()
            E[torch.arange(kb), torch.arange(kb)] = 1
            Y = torch.empty((kb, m), dtype=tdt, device="cuda").t()
            ps = timed(lambda: bsm.mul(Y, A, E))
            out["pass_ms"], out["pass_columns"] = stats(ps), kb
            med = sorted(ps)[len(ps) // 2] * 1e3
            out["route_diag_ms"] = round(-(-min(m, n) // kb) * med, 2)
            out["route_column_ms"] = round(med, 4)  # (one pass, 15 of its columns idle)
            out["route_window_ms"] = round(-(-len(idx) // kb) * med, 2)
        print(json.dumps(out), flush=True)
        del A, p
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
