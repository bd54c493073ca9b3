#!/usr/bin/env python3
"""Developer probe: the sequence of HIP runtime calls a multi-device product issues (csrc/bsm_fanout.cpp), to compare two
builds of the library call by call.  A lost wait does not fail a parity test reliably; a changed call sequence shows here.

  fanout_calls.py trace --lib LIB --out DIR   every knob setting below in a fresh child process under
                                               `rocprofv3 --hip-runtime-trace` (no counters alongside); traces in DIR/<setting>/
  fanout_calls.py compare DIR_A DIR_B          reduces each trace to the sequence of API NAMES per host thread and reports, per
                                               setting and case, the number of calls compared and the first difference
  fanout_calls.py child SETTING                (what `trace` starts) the fixed list of products of one setting

Only the names and their order are compared, per thread; arguments, timestamps and thread ids are not.  The calling thread's
sequence is cut into cases at a marker call the library never makes (hipRuntimeGetVersion, issued from here in front of every
case); the issuing threads of a five-part handle are compared as a sorted list of whole sequences (which of them starts first
is not fixed)."""
import csv, ctypes, glob, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = "hipRuntimeGetVersion"
# knob settings; "host": vectors in host memory (numpy) where a product takes them
SETTINGS = {
    "default": {},
    "flags1_own_streams": {"BSM_DIST_FLAGS": "1", "BSM_DIST_ONE_STREAM": "0"},
    "flags0_own_streams": {"BSM_DIST_FLAGS": "0", "BSM_DIST_ONE_STREAM": "0"},
    "flags0": {"BSM_DIST_FLAGS": "0"},
    "rezero0": {"BSM_DIST_REZERO": "0"},
    "rezero0_own_streams": {"BSM_DIST_REZERO": "0", "BSM_DIST_ONE_STREAM": "0"},
    "host": {},
    "copies": {"BSM_DIST_COPIES": "1"},
}


def child(setting):
    sys.path.insert(0, ROOT)
    import numpy as np, torch, bsm_amd as bsm
    S = bsm.synthetic
    host = setting == "host"
    hip = None
    with open("/proc/self/maps") as f:  # the HIP runtime torch has loaded, not a second copy of it
        for line in f:
            if "libamdhip64" in line:
                hip = ctypes.CDLL(line.split()[-1])
                break
    version = ctypes.c_int(0)
    names = []

    def case(name):
        hip.hipRuntimeGetVersion(ctypes.byref(version))
        names.append(name)

    def vec(n, K, seed, fill=None):
        rng = np.random.default_rng(seed)
        a = rng.standard_normal((n, K)) if fill is None else np.full((n, K), fill)
        if host:
            return np.asfortranarray(a) if K > 1 else a[:, 0].copy()
        t = torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()
        return t if K > 1 else t[:, 0].contiguous()

    probs = {"blocksparse": S.config1(n=600, nblocks=40, bs=16), "vbcrs": S.config2(n=6000, nblocks=300),
             "symmetric": S.config3(nseg=24)}
    for kind, prob in probs.items():
        n = prob["size"][0]
        case(f"{kind}: create P=3")
        A = S.build(prob, devices=[0, 0, 0])
        At = bsm.transpose(A)
        x1, x11 = vec(n, 1, 1), vec(n, 11, 2)
        y1, y11 = vec(n, 1, 3, fill=np.nan), vec(n, 11, 4)
        torch.cuda.synchronize()
        case(f"{kind}: mul N K=1 strong-zero beta")
        bsm.mul(y1, A, x1)
        case(f"{kind}: mul N K=1 numeric beta")
        bsm.mul(y1, A, x1, 0.5, -2.0)
        case(f"{kind}: mul T K=1 strong-zero beta")
        bsm.mul(y1, At, x1)
        case(f"{kind}: mul T K=1 numeric beta")
        bsm.mul(y1, At, x1, 0.5, -2.0)
        case(f"{kind}: mul N K=11 numeric beta")
        bsm.mul(y11, A, x11, 1.0, 0.25)
        case(f"{kind}: mul T K=11 strong-zero beta")
        bsm.mul(y11, At, x11)
        case(f"{kind}: mul N K=1 behind the wider batch")
        bsm.mul(y1, A, x1)
        parts = A.parts()
        xd = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).cuda()
        # (partitioned vectors need the fused path: not where the copy path is forced)
        for name, M, xk, yk in (("N", A, "cols", "own"), ("T", At, "own", "cols")) if setting != "copies" else ():
            xp = [xd[p[xk][0] - 1:p[xk][1]].clone() for p in parts]
            yp = [torch.zeros(max(p[yk][1] - p[yk][0] + 1, 0), dtype=xd.dtype, device="cuda") for p in parts]
            torch.cuda.synchronize()
            case(f"{kind}: mul_parts {name} strong-zero beta")
            bsm.mul_parts(yp, M, xp)
            case(f"{kind}: mul_parts {name} numeric beta")
            bsm.mul_parts(yp, M, xp, 1.0, 1.0)
        case(f"{kind}: mul N K=1 behind partitioned vectors")
        bsm.mul(y1, A, x1)
        torch.cuda.synchronize()
        case(f"{kind}: destroy")
        del At, A
    prob = probs["symmetric"]
    n = prob["size"][0]
    case("symmetric: create P=5 (issuing threads)")
    A = S.build(prob, devices=[0] * 5)
    x1, y1 = vec(n, 1, 6), vec(n, 1, 7)
    torch.cuda.synchronize()
    case("symmetric: mul N K=1 P=5 numeric beta")
    bsm.mul(y1, A, x1, 1.0, 0.5)
    case("symmetric: mul T K=1 P=5 strong-zero beta")
    bsm.mul(y1, bsm.transpose(A), x1)
    torch.cuda.synchronize()
    case("symmetric: destroy P=5")
    del A
    case("end")
    with open(os.environ["FANOUT_CASES"], "w") as f:
        json.dump(names, f)


def trace(lib, out):
    for setting, knobs in SETTINGS.items():
        d = os.path.join(out, setting)
        os.makedirs(d, exist_ok=True)
        env = dict(os.environ, BSM_LIB=os.path.abspath(lib), FANOUT_CASES=os.path.join(d, "cases.json"), **knobs)
        subprocess.run(["rocprofv3", "--hip-runtime-trace", "-f", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                        "child", setting], env=env, check=True, timeout=300)
        print(f"traced {setting}", flush=True)


def sequences(d):
    """(cases of the calling thread: [(name, [api names])], sorted sequences of the other threads)"""
    files = glob.glob(os.path.join(d, "**", "*hip_api_trace.csv"), recursive=True)
    assert len(files) == 1, (d, files)
    by_thread = {}
    with open(files[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        by_thread.setdefault(r["Thread_Id"], []).append(r["Function"])
    main = next(t for t, s in by_thread.items() if MARKER in s)
    with open(os.path.join(d, "cases.json")) as f:
        names = json.load(f)
    cases = [("start-up", [])]
    it = iter(names)
    for fn in by_thread[main]:
        if fn == MARKER:
            cases.append((next(it), []))
        else:
            cases[-1][1].append(fn)
    return cases, sorted(s for t, s in by_thread.items() if t != main)


def first_difference(a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        if u != v:
            return i
    return None if len(a) == len(b) else min(len(a), len(b))


def compare(da, db):
    ok, total = True, 0
    for setting in SETTINGS:
        (ca, ta), (cb, tb) = sequences(os.path.join(da, setting)), sequences(os.path.join(db, setting))
        ncalls, diffs = 0, []
        if [n for n, _ in ca] != [n for n, _ in cb]:
            diffs.append("different case lists")
        for (name, sa), (_, sb) in zip(ca[1:], cb[1:]):  # (start-up: torch's own initialisation, before the first case)
            ncalls += len(sa)
            i = first_difference(sa, sb)
            if i is not None:
                diffs.append(f"case '{name}': call {i}: {sa[max(i - 3, 0):i + 2]} against {sb[max(i - 3, 0):i + 2]} "
                             f"({len(sa)} / {len(sb)} calls)")
        nthread = sum(len(s) for s in ta)
        if ta != tb:
            diffs.append(f"other threads: {len(ta)} / {len(tb)} threads, {nthread} / {sum(len(s) for s in tb)} calls differ")
        total += ncalls + nthread
        ok = ok and not diffs
        print(f"{setting}: {len(ca) - 1} cases, {ncalls} calls on the calling thread, {nthread} on {len(ta)} other threads: "
              f"{'equal' if not diffs else 'DIFFERENT'}")
        for d in diffs:
            print("   " + d)
    print(f"{total} calls compared by name and order (arguments are not compared): {'equal' if ok else 'DIFFERENT'}")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2])
    elif sys.argv[1] == "trace":
        trace(sys.argv[sys.argv.index("--lib") + 1], sys.argv[sys.argv.index("--out") + 1])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
