#!/usr/bin/env python3
"""Developer probe: which kernels a product launches, in which order -- one small operator per image class of the
multi-column policy (csrc/bsm_plan.cpp) and per (stored type, vector type) pair, the product for K = 1 ... 35, ops N and
T, eagerly and then all of them once inside a captured graph (which does not get the interleaved pass's work arrays).
Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/plan_sweep.py` with two builds
(BSM_LIB) and compare the ordered launches with tools/kt_order_diff.py DIR_A DIR_B."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, bsm_amd as bsm
from _common import fixture_problem
S = bsm.synthetic
torch.cuda.set_device(0)
print(bsm._lib.LIB_PATH, bsm._lib.lib().bsm_version().decode(), flush=True)
f64, f32, c128, c64 = np.float64, np.float32, np.complex128, np.complex64
TT = {np.dtype(f64): torch.float64, np.dtype(f32): torch.float32, np.dtype(c128): torch.complex128, np.dtype(c64): torch.complex64}
ops = [
    # (name, problem, build kw, vector dtype)
    ("excl fwd vbcrs f64", S.config2(n=6000, nblocks=300), {}, f64),
    ("excl fwd vbcrs short f64", S.config2(n=3000, nblocks=300, lo=4, hi=24), {}, f64),
    ("excl fwd vbcrs f32", S.config2(n=6000, nblocks=300, dtype=f32), {}, f32),
    ("excl fwd vbcrs c128", S.config2(n=6000, nblocks=300, dtype=c128), {}, c128),
    ("excl fwd vbcrs mixed", S.config2(n=6000, nblocks=300), {"storage": f32}, f64),
    ("excl fwd vbcrs cvec", S.config2(n=6000, nblocks=300), {}, c128),
    ("fwd acc short f64", S.config1(n=1000, nblocks=50, bs=16), {"accumulate": "atomic"}, f64),
    ("fwd acc short c64", S.config1(n=1000, nblocks=50, bs=16, dtype=c64), {"accumulate": "atomic"}, c64),
    ("fwd acc tall f64", S.config1(n=1000, nblocks=50, bs=64), {"accumulate": "atomic"}, f64),
    ("fwd acc tall f32", S.config1(n=1000, nblocks=50, bs=64, dtype=f32), {"accumulate": "atomic"}, f32),
    ("fwd acc tall mixed", S.config1(n=1000, nblocks=50, bs=64), {"accumulate": "atomic", "storage": f32}, f64),
    ("sym short f64", S.config3(nseg=40, bs=16, halfband=3), {}, f64),
    ("sym short c128 (fixture)", fixture_problem("cuboid"), {}, c128),
    ("sym short c128 mixed", fixture_problem("cuboid"), {"storage": c64}, c128),
    ("sym tall f64", S.config3(nseg=24), {}, f64),
    ("sym tall f32", S.config3(nseg=24, dtype=f32), {}, f32),
    ("sym tall c128", S.config3(nseg=24, dtype=c128), {}, c128),
    ("sym tall c64", S.config3(nseg=24, dtype=c64), {}, c64),
    ("sym tall mixed", S.config3(nseg=24), {"storage": f32}, f64),
    ("sym tall cvec", S.config3(nseg=24), {}, c128),
    ("sym tall f32 cvec", S.config3(nseg=24, dtype=f32), {}, c64),
    ("coloured sym f64", S.config3(nseg=40, bs=16, halfband=3), {"accumulate": "colored"}, f64),
    ("coloured blocksparse f64", S.config1(n=1000, nblocks=50, bs=16), {"accumulate": "colored"}, f64),
]
KS = range(1, 36)
nprod = 0
for name, p, kw, vt in ops:
    try:
        A = S.build(p, **kw)
    except RuntimeError as e:
        print("SKIPPED", name, e, flush=True)
        continue
    m, n = p["size"]
    tt = TT[np.dtype(vt)]
    before = A.value_passes()
    g = torch.Generator(device="cuda").manual_seed(5)
    def vec(k, ln):
        if k == 1:
            return torch.randn(ln, dtype=tt, device="cuda", generator=g)
        return torch.randn((k, ln), dtype=tt, device="cuda", generator=g).t()
    work = []
    for opname in "NT":
        Aop = A if opname == "N" else bsm.transpose(A)
        xl, yl = (n, m) if opname == "N" else (m, n)
        for k in KS:
            work.append((Aop, vec(k, xl), vec(k, yl)))
    for Aop, X, Y in work:  # eagerly
        bsm.mul(Y, Aop, X, 0.5, 2.0)
        nprod += 1
    torch.cuda.synchronize()
    eager = A.value_passes() - before
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):  # (a captured product must not get the work arrays)
            for Aop, X, Y in work:
                bsm.mul(Y, Aop, X, 0.5, 2.0)
                nprod += 1
    torch.cuda.current_stream().wait_stream(s)
    captured = A.value_passes() - before - eager
    gr.replay()
    torch.cuda.synchronize()
    print(f"{name}: value passes eager {eager}, captured {captured}", flush=True)
    del gr, work, A
print("products", nprod, flush=True)
