#!/usr/bin/env python3
"""Developer probe: the device assembly (`make asm`) of two trees compared kernel by kernel, keyed by symbol -- for
changes that move kernels between translation units and must leave their code alone.  Each side is any number of .s
files; a file is cut at the function boundaries, the function number is stripped from local labels (.LBB<f>_<n>,
.Lfunc_end<f>; any other numbered local label form is reported), and a symbol's text is its instructions (comments dropped) plus its
kernel descriptor (.amdhsa_kernel block and the .set <symbol>.* resource lines).
usage: asm_symbol_diff.py A.s [A2.s ...] -- B.s [B2.s ...]      exit status 1: symbols on one side only or differing"""
import re, sys, collections
LABEL = re.compile(r"\.L[A-Za-z_]+\d*(?:_\d+)?")
def norm(line, odd):
    def fix(m):
        t = m.group(0)
        if re.fullmatch(r"\.LBB\d+_\d+", t): return ".LBB_" + t.split("_")[1]
        if re.fullmatch(r"\.Lfunc_end\d+", t): return ".Lfunc_end"
        if re.search(r"\d", t): odd[re.sub(r"\d+", "N", t)] += 1
        return t
    return LABEL.sub(fix, line)
def load(files):
    body, desc, odd = {}, collections.defaultdict(list), collections.Counter()
    for f in files:
        cur = kd = None
        for line in open(f):
            line = line.rstrip()
            m = re.match(r"(\S+):\s*; @(\S+)$", line)
            if m and m.group(1) == m.group(2):
                cur = m.group(1)
                if cur in body: sys.exit(f"{f}: {cur} defined twice on one side")
                body[cur] = []
                continue
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m: kd = m.group(1)
            if kd is not None:  # (the descriptor sits inside the function's text, in front of .Lfunc_end)
                desc[kd].append(line.strip())
                if line.strip() == ".end_amdhsa_kernel": kd = None
                continue
            if cur is not None:
                code = norm(line.split(";")[0].rstrip(), odd)  # (comments name basic blocks by function number too)
                if code: body[cur].append(code)
                if re.match(r"\.Lfunc_end\d+:", line): cur = None
                continue
            m = re.match(r"\s*\.set (\S+?)\.(\w+), (.*)", line)
            if m and m.group(1) in body: desc[m.group(1)].append(f"{m.group(2)} = {m.group(3)}")
    return body, desc, odd
sep = sys.argv.index("--")
(ba, da, oa), (bb, db, ob) = load(sys.argv[1:sep]), load(sys.argv[sep + 1:])
only_a, only_b = sorted(set(ba) - set(bb)), sorted(set(bb) - set(ba))
both = sorted(set(ba) & set(bb))
dbody = [s for s in both if ba[s] != bb[s]]
ddesc = [s for s in both if da[s] != db[s]]
print(f"symbols: a {len(ba)}, b {len(bb)}, common {len(both)}; kernel descriptors: a {sum(1 for s in da if any(l.startswith('.amdhsa_kernel') for l in da[s]))}, "
      f"b {sum(1 for s in db if any(l.startswith('.amdhsa_kernel') for l in db[s]))}")
print(f"only in a: {len(only_a)}  only in b: {len(only_b)}  differing bodies: {len(dbody)}  differing descriptors: {len(ddesc)}")
print("other function-numbered label forms:", dict(oa + ob) or "none")
for tag, l in (("only in a", only_a), ("only in b", only_b), ("body differs", dbody), ("descriptor differs", ddesc)):
    for s in l: print(f"  {tag}: {s}")
sys.exit(1 if only_a or only_b or dbody or ddesc else 0)
