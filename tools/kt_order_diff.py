#!/usr/bin/env python3
"""Developer probe: the kernel launches of two `rocprofv3 --kernel-trace --output-format csv` runs as ordered lists of
(kernel name, grid size), and whether they are identical.  usage: kt_order_diff.py DIR_A DIR_B [OUTDIR for the two lists]"""
import csv, glob, sys, collections
def load(d):
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))))
    rows.sort()
    return [(n, g) for _, n, g in rows]
a, b = load(sys.argv[1]), load(sys.argv[2])
for tag, l in (("a", a), ("b", b)) if len(sys.argv) > 3 else ():
    with open(sys.argv[3] + "/" + tag + "_launches.txt", "w") as f:
        for n, g in l:
            f.write(f"{g[0]},{g[1]},{g[2]} {n}\n")
bsm_a = sum(1 for n, _ in a if "bsm::" in n)
print(f"launches: a {len(a)} ({bsm_a} of the library's kernels), b {len(b)} ({sum(1 for n, _ in b if 'bsm::' in n)})")
diff = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
print("ordered lists identical:", a == b, "first differences:", [(i, a[i], b[i]) for i in diff[:5]])
print("as multisets identical:", collections.Counter(a) == collections.Counter(b))
print("distinct library kernels launched:", len(set(n for n, _ in a if "bsm::" in n)))
sys.exit(0 if a == b else 1)
