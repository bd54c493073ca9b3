#!/usr/bin/env python3
"""Developer probe: bsm_update_blocks against destroy + create of the same operator.

Per operator (C2, the 1.08 GB C2-shaped VBCRS leg of bench.py, C3, a C5 slice) and per block residence (device: the
operator generated in HBM, `refresh` of the mirror's own CUDA tensors; host: numpy blocks, staged):
  create_ms     destroy + create of a handle from the same blocks (host clock after a device synchronise, 2nd of 2)
  update_ms     full update through the C ABI with the pointer arrays built once (what a binding that caches them
                pays), warmed (device: hip events around `reps` back-to-back updates; host: host clock)
  subset_ms     the same for 1 % of the blocks (random ids)
  mirror_ms     full update through the Python mirror (bsm.refresh: the pointer arrays rebuilt in Python per call)
  first_ms      the FIRST update of the handle (C ABI, host clock after a device synchronise): derives the refill plan
                (re-runs the value-blind analysis on the kept block list) and uploads it, then refills
  ratio         create_ms / update_ms
One JSON line per (operator, residence).  Kernel time: run it again under
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python3 tools/update_bench.py --quick
and read refill_kernel / pack_kernel from the stats file (tools/kt_summary.py); value bytes per second =
stored_entries * element bytes / kernel time (printed here as value_bytes).
usage: update_bench.py [--quick] [--only c2,c2_1gb,c3,c5s] [--host]"""
import argparse
import json
import os
import sys
import time

import ctypes as C

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsm_amd as bsm  # noqa: E402
from bsm_amd import _lib as L  # noqa: E402

S = bsm.synthetic
OPS = {"c2": lambda d: S.config2(on_device=d), "c2_1gb": lambda d: S.config2(n=2_000_000, nblocks=100_000, on_device=d),
       "c3": lambda d: S.config3(on_device=d), "c5s": lambda d: S.config5(n=625_000, on_device=d)}
ES = {np.dtype(np.float32): 4, np.dtype(np.float64): 8, np.dtype(np.complex64): 8, np.dtype(np.complex128): 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions (kernel-trace runs)")
    ap.add_argument("--only", default="c2,c2_1gb,c3,c5s")
    ap.add_argument("--host", action="store_true", help="also host-resident blocks")
    a = ap.parse_args()
    import torch
    reps = 3 if a.quick else 10
    rng = np.random.default_rng(0)
    for name in a.only.split(","):
        for where in (("device", "host") if a.host else ("device",)):
            p = OPS[name](where == "device")
            torch.cuda.synchronize()
            A = None
            create = []
            for _ in range(2):
                del A
                torch.cuda.synchronize()
                t = time.perf_counter()
                A = S.build(p)
                torch.cuda.synchronize()
                create.append(time.perf_counter() - t)
            st = A.stats()
            nb = len(A._src())
            value_bytes = st["stored_entries"] * ES[np.dtype(A.dtype)]
            ids = list(rng.choice(nb, size=max(1, nb // 100), replace=False) + 1)

            def timed(fn):
                if where == "device":
                    fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1) / reps
                fn()
                t = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t) / reps * 1e3
            src = A._src()
            devb = where == "device"
            ptrs = (C.c_void_p * nb)(*[(b.data_ptr() if devb else b.ctypes.data) for b in src])
            lds = np.ascontiguousarray([max(b.stride(1) if devb else b.shape[0], b.shape[0], 1) for b in src], dtype=np.int64)
            sid = np.ascontiguousarray(ids, dtype=np.int64)
            sptrs = (C.c_void_p * len(ids))(*[ptrs[i - 1] for i in ids])
            slds = np.ascontiguousarray(lds[sid - 1])
            I = C.POINTER(C.c_int64)
            ms = L.BSM_MEM_DEVICE if devb else L.BSM_MEM_HOST
            stream = torch.cuda.current_stream().cuda_stream if devb else None

            def raw_full():
                L.check(L.lib().bsm_update_blocks(A._h.ptr, nb, None, ptrs, lds.ctypes.data_as(I), ms, stream))

            def raw_sub():
                L.check(L.lib().bsm_update_blocks(A._h.ptr, len(ids), sid.ctypes.data_as(I), sptrs, slds.ctypes.data_as(I),
                                                  ms, stream))
            torch.cuda.synchronize()
            t = time.perf_counter()
            raw_full()  # first update: plan derivation + upload
            torch.cuda.synchronize()
            first_ms = (time.perf_counter() - t) * 1e3
            full_ms = timed(raw_full)
            sub_ms = timed(raw_sub)
            mirror_ms = timed(lambda: bsm.refresh(A))
            print(json.dumps({"op": name, "blocks": where, "nblocks": nb, "value_bytes": value_bytes,
                              "create_ms": round(create[-1] * 1e3, 3), "update_ms": round(full_ms, 4),
                              "subset_ms": round(sub_ms, 4), "subset_blocks": len(ids), "mirror_ms": round(mirror_ms, 3),
                              "first_ms": round(first_ms, 2),
                              "ratio": round(create[-1] * 1e3 / full_ms, 1),
                              "update_value_GBps": round(value_bytes / (full_ms * 1e-3) / 1e9, 1)}), flush=True)
            del A, p
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
