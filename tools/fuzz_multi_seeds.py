#!/usr/bin/env python3
"""Developer probe: the multi-RHS part of tests/test_gpu_fuzz.py over OTHER seeds (the suite's own seeds are fixed):
random operators of the three types and four element types, every accumulation mode, ops N / T / C, 2-35 columns,
complex scalars for the complex types, every column against the oracle.
usage: fuzz_multi_seeds.py [first seed] [count] [--digest OUT.json]
       fuzz_multi_seeds.py --diff A.json B.json [C.json]
--digest also writes the sha256 of every result matrix, keyed by seed, kind, dtype, case, accumulate, op, k and the
handle's stats()["exclusive"] -- for bit comparisons between builds (BSM_LIB), one fresh process per file.  It adds
forward products of exclusive handles (plain stores, fixed-order combine; synthetic.config2 with 6 000 rows in the four
element types, 4-24 columns; digests only): the generators of the fuzz never give one, their row groups overlap.
--diff A B compares two such files case by case.  --diff A B C compares C against A on the cases where A and B (two runs
of one build) agree, and lists the others by count: sums that leave as atomics have no fixed order.  exit status 1:
differing digests, or an exclusive forward product among the cases A and B disagree on."""
import hashlib, json, os, sys, zlib


def diff(files):
    runs = [json.load(open(f)) for f in files]
    a, new = runs[0], runs[-1]
    if set(a) != set(new) or set(a) != set(runs[1]):
        sys.exit("the files hold different cases")
    if len(runs) == 2:
        bad = [c for c in a if a[c] != new[c]]
        print(f"{len(a)} cases, {len(bad)} differ")
        for c in bad: print("DIFFERS", c)
        sys.exit(1 if bad else 0)
    stable = [c for c in a if a[c] == runs[1][c]]
    loose = [c for c in a if a[c] != runs[1][c]]
    bad = [c for c in stable if a[c] != new[c]]
    # key: seed|kind|dtype|case|accumulate|op|k|exclusive
    loose_excl_fwd = [c for c in loose if c.split("|")[5] == "N" and c.split("|")[7] == "1"]
    by_mode = {}
    for c in loose:
        by_mode[c.split("|")[4]] = by_mode.get(c.split("|")[4], 0) + 1
    print(f"{len(a)} cases; {len(stable)} compared, {len(bad)} differ; {len(loose)} not reproducible between {files[0]} and {files[1]}"
          f" (by accumulate mode: {by_mode or 'none'}; exclusive forward products among them: {len(loose_excl_fwd)})")
    for c in bad: print("DIFFERS", c)
    for c in loose_excl_fwd: print("NOT REPRODUCIBLE (exclusive forward)", c)
    sys.exit(1 if bad or loose_excl_fwd else 0)


if "--diff" in sys.argv:
    diff(sys.argv[sys.argv.index("--diff") + 1:])
digest_out = None
if "--digest" in sys.argv:
    i = sys.argv.index("--digest")
    digest_out = sys.argv[i + 1]
    del sys.argv[i:i + 2]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, bsm_amd as bsm
from oracle import load_oracle
from _common import Cc, N, T, oracle_mul, rand_vec
from _fuzz import GEN
orc = load_oracle()
TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12, np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-5}
first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 6
bad = done = 0
digests = {}
for seed in range(first, first + count):
    for kind in ("blocksparse", "vbcrs", "symmetric"):
        for dtype in (np.float64, np.complex128, np.float32, np.complex64):
            dtype = np.dtype(dtype)
            rng = np.random.default_rng(seed * 1000 + zlib.crc32((kind + dtype.str).encode()) % 997)
            for case in range(8):
                p = GEN[kind](rng, dtype)
                modes = ["auto", "atomic", "gather"] + (["colored"] if kind != "vbcrs" else [])
                acc = modes[case % len(modes)]
                kw = {"accumulate": acc}
                if kind != "symmetric" and case % 3 == 0:
                    kw["transpose_image"] = True
                try:
                    A = bsm.synthetic.build(p, **kw)
                except RuntimeError as e:
                    if acc == "colored" and "repeat" in str(e):
                        continue
                    raise
                nr, nc = p["size"]
                for op in (N, T, Cc):
                    if op == Cc and dtype.kind != "c":
                        continue
                    xl, yl = (nc, nr) if op == N else (nr, nc)
                    Aop = A if op == N else (bsm.transpose(A) if op == T else bsm.adjoint(A))
                    k = int(rng.choice([2, 3, 4, 5, 7, 8, 9, 11, 15, 16, 17, 24, 35]))
                    X = np.asfortranarray(np.stack([rand_vec(rng, xl, dtype) for _ in range(k)], axis=1))
                    Y0 = np.asfortranarray(np.stack([rand_vec(rng, yl, dtype) for _ in range(k)], axis=1))
                    am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if dtype.kind == "c" else (-0.5, 1.25)
                    strong = bool(rng.integers(0, 2))
                    Yd = torch.from_numpy(Y0.T.copy()).cuda().T
                    bsm.mul(Yd, Aop, torch.from_numpy(X.T.copy()).cuda().T, am, False if strong else bm)
                    got = Yd.cpu().numpy()
                    if digest_out:
                        opn = "N" if op == N else ("T" if op == T else "C")
                        key = f"{seed}|{kind}|{dtype.name}|{case}|{acc}|{opn}|{k}|{int(bool(A.stats()['exclusive']))}"
                        digests[key] = hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()
                    for j in range(k):
                        ref = oracle_mul(orc, p, op, X[:, j].copy(), Y0[:, j].copy(), am, bm, strong)
                        err = np.max(np.abs(got[:, j] - ref)) / max(np.max(np.abs(ref)), 1e-30)
                        done += 1
                        if not err < TOL[dtype]:
                            bad += 1
                            print("MISMATCH", seed, kind, dtype, case, acc, op, k, j, err, flush=True)
    if digest_out:  # exclusive handles (digests only: the fuzz generators' row groups overlap, their handles never are)
        for dtype in (np.float64, np.complex128, np.float32, np.complex64):
            dtype = np.dtype(dtype)
            p = bsm.synthetic.config2(n=6000, nblocks=300, dtype=dtype.type, seed=seed)
            A = bsm.synthetic.build(p)
            r2 = np.random.default_rng([seed, zlib.crc32(dtype.str.encode())])
            am, bm = (-0.5 + 0.75j, 1.25 - 0.5j) if dtype.kind == "c" else (-0.5, 1.25)
            for k in (4, 5, 8, 11, 16, 24):
                X = np.asfortranarray(np.stack([rand_vec(r2, 6000, dtype) for _ in range(k)], axis=1))
                Y0 = np.asfortranarray(np.stack([rand_vec(r2, 6000, dtype) for _ in range(k)], axis=1))
                Yd = torch.from_numpy(Y0.T.copy()).cuda().T
                bsm.mul(Yd, A, torch.from_numpy(X.T.copy()).cuda().T, am, bm)
                digests[f"{seed}|c2|{dtype.name}|0|auto|N|{k}|{int(bool(A.stats()['exclusive']))}"] = \
                    hashlib.sha256(np.ascontiguousarray(Yd.cpu().numpy()).tobytes()).hexdigest()
    print(f"seed {seed}: {done} columns checked, {bad} mismatches", flush=True)
if digest_out:
    json.dump(digests, open(digest_out, "w"), indent=0, sort_keys=True)
    print(f"{len(digests)} digests -> {digest_out}")
sys.exit(1 if bad else 0)
