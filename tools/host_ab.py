#!/usr/bin/env python3
"""Developer probe: host cost of the Python layer, A/B between two checkouts of it against ONE libbsmrocm.so.
usage: host_ab.py PARENT_ROOT NEW_ROOT [reps=5]   (BSM_LIB: the library both use; default NEW_ROOT's)

Alternates PARENT, NEW, PARENT, NEW ... in fresh child processes; each child imports bsm_amd from its root and times
  mul1 / mul8   eager bsm.mul on device tensors, 1 and 8 columns, on an 8 x 8 operator of two 4 x 4 blocks: the host, not the
                kernel, bounds the loop (5000 calls, one synchronise) -- us per call
  plan_c2       tools/hostpath.py's device-resident figure: MulPlan on C2, 300 calls, one synchronise -- us per call
  create_c2/c3  tools/createtime.py's figure for c2 and c3: the second of two builds on the device -- seconds
The verdict per figure: NEW's median against PARENT's min .. max of the same run."""
import json
import os
import statistics
import subprocess
import sys
import time


def child(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import bsm_amd as bsm
    assert os.path.dirname(os.path.abspath(bsm.__file__)).startswith(os.path.abspath(root)), bsm.__file__
    out = {}

    def loop(call, n, warm):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    idx = [[1, 2, 3, 4], [5, 6, 7, 8]]
    A = bsm.BlockSparseMatrix([np.asfortranarray(np.arange(16.0).reshape(4, 4)) for _ in range(2)], idx, idx, (8, 8))
    x, y = torch.ones(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    X, Y = torch.ones((8, 8), dtype=torch.float64, device="cuda").t(), torch.zeros((8, 8), dtype=torch.float64, device="cuda").t()
    out["mul1"] = loop(lambda: bsm.mul(y, A, x), 5000, 500)
    out["mul8"] = loop(lambda: bsm.mul(Y, A, X), 5000, 500)
    S = bsm.synthetic
    built = {}
    for name, mk in (("c2", S.config2), ("c3", S.config3)):
        p = mk()
        for rep in range(2):
            t0 = time.perf_counter()
            B = S.build(p)
            out["create_" + name] = time.perf_counter() - t0
        built[name] = (p, B)
    p, B = built["c2"]
    xd, yd = torch.from_numpy(p["x"]).cuda(), torch.zeros(len(p["x"]), dtype=torch.float64, device="cuda")
    out["plan_c2"] = loop(bsm.MulPlan(yd, B, xd), 300, 10)
    print("HOSTAB " + json.dumps(out), flush=True)


def main():
    parent, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    env = dict(os.environ)
    env.setdefault("BSM_LIB", os.path.join(new, "blocksparsematrices.jl_amd", "libbsmrocm.so"))
    runs = {"parent": [], "new": []}
    for rep in range(reps):
        for side, root in (("parent", parent), ("new", new)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], env=env, capture_output=True, text=True,
                                 timeout=600)
            line = [l for l in res.stdout.splitlines() if l.startswith("HOSTAB ")]
            if res.returncode or not line:
                sys.exit(f"{side} child failed ({res.returncode}):\n{res.stdout}\n{res.stderr}")
            runs[side].append(json.loads(line[0][7:]))
            print(side, rep, line[0][7:], flush=True)
    for key in runs["parent"][0]:
        a, b = [r[key] for r in runs["parent"]], [r[key] for r in runs["new"]]
        med = statistics.median(b)
        verdict = "within" if min(a) <= med <= max(a) else ("below" if med < min(a) else "ABOVE")
        print(f"{key:10s} parent min {min(a):.4g} median {statistics.median(a):.4g} max {max(a):.4g} | new min {min(b):.4g} "
              f"median {med:.4g} max {max(b):.4g} -> new median {verdict} the parent's range")


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
