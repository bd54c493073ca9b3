#!/usr/bin/env python3
"""Developer probe: WHERE the workgroups of one C2 launch run (trace build, make -C csrc trace -> libbsmrocm_trace.so:
every wave stamps HW_ID and XCC_ID beside its timestamps) and what a compute unit's finish time follows.
  1. the placement rule workgroup index -> XCD / SE / CU, and whether it repeats: 20 single launches, 5 back-to-back
     runs, one graph replay
  2. per CU: workgroups, bytes, lane-padded bytes (bytes x P / m), iterations, time of its last store
  3. which of those predicts the last-store time best (least squares, one predictor at a time)
usage: BSM_LIB=.../libbsmrocm_trace.so [BSM_ORDER=..] tools/placement_census.py [c2|c2w] [--raw FILE]"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, bsm_amd as bsm
from bsm_amd import _lib
from _common import get_image, WORK_PANEL
args = [a for a in sys.argv[1:]]
raw = args[args.index("--raw") + 1] if "--raw" in args else None
which = args[0] if args and not args[0].startswith("--") else "c2"
S = bsm.synthetic
p = {"c2": S.config2, "c2w": lambda: S.config2(n=100000, lo=64, hi=64, nblocks=1650)}[which]()
A = S.build(p)
st = A.stats()
nwg = st["nworkgroups"]
nw = nwg * 4
waves = get_image(S.build(p, device=-2))[3]  # the wave records: an analysis-only twin (same knobs, same CU count)
assert len(waves) == nw

# per-workgroup cost measures from the wave records
panel = (waves["work"] == WORK_PANEL) & (waves["npieces"] > 0)
m = waves["m"].astype(np.int64)
lanes = np.where(m <= 8, 8, np.where(m <= 16, 16, np.where(m <= 32, 32, 64)))
wbytes = np.where(panel, waves["first"]["nstrips"].astype(np.int64) * m * 16, 0)
wpad = np.where(panel, waves["first"]["nstrips"].astype(np.int64) * lanes * 16, 0)
wit = -(-wbytes // 8192)
wg_bytes = wbytes.reshape(nwg, 4).sum(1)
wg_pad = wpad.reshape(nwg, 4).sum(1)
wg_it = wit.reshape(nwg, 4).sum(1)
wg_itmax = wit.reshape(nwg, 4).max(1)

x = torch.from_numpy(p["x"]).cuda(); y = torch.zeros_like(x)
plan = bsm.MulPlan(y, A, x)
for _ in range(20):
    plan()
torch.cuda.synchronize()
buf = torch.zeros(nw * 16, dtype=torch.int64, device="cuda")
L = _lib.lib()
L.bsm_debug_set_trace.argtypes = [C.c_void_p]
assert L.bsm_debug_set_trace(buf.data_ptr()) == 0


def read():
    """-> (cu key per workgroup, last-store time per workgroup in us on the chip-wide clock, trace rows)"""
    t = buf.cpu().numpy().reshape(nw, 16)
    hw, xcc = t[:, 9], t[:, 10] & 15
    cu, sh, se = (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    key = (((xcc * 8 + se) * 2 + sh) * 16 + cu).reshape(nwg, 4)
    assert (key == key[:, :1]).all(), "the waves of a workgroup share a CU"
    stored = ((t[:, 8] - t[:, 7].min()) / 100.0).reshape(nwg, 4).max(1)
    return key[:, 0].copy(), stored, t


def fmt(k):
    return "x%d.se%d.sh%d.cu%02d" % (k >> 8, (k >> 5) & 7, (k >> 4) & 1, k & 15)


print(f"{which}: {nwg} workgroups, {wg_bytes.sum()/1e6:.2f} MB, BSM_ORDER={os.environ.get('BSM_ORDER', 'default')}, build {L.bsm_version().decode()}")
# ---- 1. placement: single launches, back-to-back runs, a graph replay ------------------------------------------
single = []
for rep in range(20):
    buf.zero_(); plan(); torch.cuda.synchronize()
    single.append(read()[0])
b2b, b2b_t = [], []
for rep in range(5):
    buf.zero_()
    for _ in range(50):  # the buffer keeps the LAST launch: clocks and caches as in the benchmark
        plan()
    torch.cuda.synchronize()
    k, s, _ = read()
    b2b.append(k); b2b_t.append(s)
graph = None
try:
    s_ = torch.cuda.Stream(); s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s_):
            for _ in range(50):
                plan()
    torch.cuda.current_stream().wait_stream(s_)
    g.replay(); torch.cuda.synchronize()
    buf.zero_(); g.replay(); torch.cuda.synchronize()
    graph, graph_t, _ = read()
except Exception as e:  # capture not available
    print("graph replay: not available (%r)" % (e,))
ref = single[0]
same = lambda a, b: float((a == b).mean())
print("placement, share of workgroups on the SAME CU as in the first single launch:")
print("  20 single launches : " + " ".join("%.3f" % same(ref, k) for k in single[1:]))
print("  5 back-to-back runs: " + " ".join("%.3f" % same(ref, k) for k in b2b))
if graph is not None:
    print("  graph replay       : %.3f" % same(ref, graph))
print("  same XCD           : single %.3f  back-to-back %.3f" % (np.mean([same(ref >> 8, k >> 8) for k in single[1:]]),
                                                                np.mean([same(ref >> 8, k >> 8) for k in b2b])))
idx = np.arange(nwg)
print("  XCD == workgroup index mod 8: %.3f (first launch), %.3f (last back-to-back run)" % (same(ref >> 8, idx % 8), same(b2b[-1] >> 8, idx % 8)))
cus = np.unique(np.concatenate(single + b2b + ([graph] if graph is not None else [])))
print(f"  {len(cus)} distinct CUs seen; per XCD: " + " ".join(str(int(((cus >> 8) == xc).sum())) for xc in range(8)))
for name, k in (("first single launch", ref), ("last back-to-back run", b2b[-1])):
    print(f"  {name}: workgroups 0..63 of XCD 0 (index 0, 8, 16, ..) ->")
    sel = k[0:512:8]
    for r0 in range(0, 64, 8):
        print("    " + " ".join(fmt(v)[3:] for v in sel[r0:r0 + 8]))
    # position of a workgroup among its XCD's CUs: does slot j of an XCD's sequence return to the same CU every 32?
    seq = k[0::8]
    per = [same(seq[:len(seq) - d], seq[d:]) for d in (16, 32, 36, 64)]
    print("    XCD 0: share of workgroups on the same CU as the one 16 / 32 / 36 / 64 places earlier: " + " ".join("%.3f" % v for v in per))
    cnt = np.bincount(np.searchsorted(cus, k), minlength=len(cus))
    print("    workgroups per CU: " + " ".join(f"{int(c)}:{int((cnt == c).sum())}" for c in np.unique(cnt)))

# ---- 2. per CU of the last back-to-back run ---------------------------------------------------------------------
def per_cu(k, stored):
    pos = np.searchsorted(cus, k)
    n = len(cus)
    out = {"wgs": np.bincount(pos, minlength=n).astype(float), "bytes": np.bincount(pos, wg_bytes, n), "padded": np.bincount(pos, wg_pad, n),
           "iters": np.bincount(pos, wg_it, n), "itmax": np.zeros(n)}
    last = np.zeros(n)
    np.maximum.at(last, pos, stored)
    np.maximum.at(out["itmax"], pos, wg_itmax.astype(float))
    return out, last


print("per CU (last back-to-back run; mean / max / max over mean):")
q, last = per_cu(b2b[-1], b2b_t[-1])
for nm, v in q.items():
    print(f"  {nm:7s} mean {v.mean():10.1f}  max {v.max():10.1f}  max/mean {v.max()/v.mean():.3f}")
print(f"  last store: min {last.min():.2f}  p10 {np.percentile(last,10):.2f}  p50 {np.percentile(last,50):.2f}  p90 {np.percentile(last,90):.2f}  max {last.max():.2f} us"
      f"  (spread p90 - p10 {np.percentile(last,90)-np.percentile(last,10):.2f}, max - p50 {last.max()-np.percentile(last,50):.2f})")
xl = np.array([last[(cus >> 8) == xc].max() for xc in range(8)])
xb = np.array([q["bytes"][(cus >> 8) == xc].sum() for xc in range(8)])
print("  per XCD: bytes (MB) " + " ".join("%.2f" % (b / 1e6) for b in xb) + " ; last store (us) " + " ".join("%.2f" % v for v in xl))

# ---- 3. what predicts a CU's last store: one predictor at a time, over the 5 back-to-back runs ---------------------
print("least squares last_store = a + b * measure, per CU, pooled over the 5 back-to-back runs (and the graph replay):")
runs = list(zip(b2b, b2b_t)) + ([(graph, graph_t)] if graph is not None else [])
for nm in ("wgs", "bytes", "padded", "iters", "itmax"):
    X, Y = [], []
    for k, s in runs:
        qq, ll = per_cu(k, s)
        X.append(qq[nm]); Y.append(ll - ll.mean())
    X, Y = np.concatenate(X), np.concatenate(Y)
    Am = np.stack([np.ones_like(X), X], 1)
    coef, *_ = np.linalg.lstsq(Am, Y, rcond=None)
    r = Y - Am @ coef
    r2 = 1 - (r @ r) / ((Y - Y.mean()) @ (Y - Y.mean()))
    print(f"  {nm:7s} slope {coef[1]:.4g} us per unit   R^2 {r2:.3f}   corr {np.corrcoef(X, Y)[0,1]:.3f}")
# the late stores: are they on the loaded CUs?
k, s = b2b[-1], b2b_t[-1]
late = np.argsort(s)[-16:]
pos = np.searchsorted(cus, k)
print("the 16 workgroups that store last (last back-to-back run): index, bytes, iterations, its CU's bytes / mean, stored at")
for i in late[::-1]:
    print(f"  wg {i:5d}  {wg_bytes[i]:7d} B  it {wg_it[i]:2d} (max {wg_itmax[i]})  CU {fmt(k[i])} load {q['bytes'][pos[i]]/q['bytes'].mean():.2f}  {s[i]:.2f} us")
if raw:
    np.savez_compressed(raw, single=np.array(single), b2b=np.array(b2b), b2b_t=np.array(b2b_t), graph=graph if graph is not None else np.zeros(0),
                        wg_bytes=wg_bytes, wg_pad=wg_pad, wg_it=wg_it, wg_itmax=wg_itmax, cus=cus)
