"""Diagnostic: where does a PCG iteration of the resident kernel spend its time?
   ARAPOPT_STAMPS=1 python tools/res_stamps.py [batch]   (instrumented build; never quote its run time)"""
import os, sys, time
os.environ["ARAPOPT_STAMPS"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from arap_flow_amd import opt, synth
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
full = len(sys.argv) > 2 and sys.argv[2] == "full"
W, H, L = 854, 480, 400
st = opt.State()
fs = opt.FrameSolver(st, W, H, batch=B)
for b in range(B):
    f = synth.make_frame(W, H, seed=b, full_mask=full)
    fs.set_frame(b, f["mask_red"], f["constraints"])
fs.solve(B, 1, 2, L)
torch.cuda.synchronize()
t = time.perf_counter(); fs.solve(B, 1, 4, L); torch.cuda.synchronize(); dt = time.perf_counter() - t
out = np.zeros((512, 16), np.uint64)
assert st.lib.ArapFlow_SolverStamps(fs.h, out.ctypes.data) == 0
o = out.astype(np.float64)
used = o[:, 0] > 0
us = o[used, :5] * 0.01 / L          # 100 MHz ticks -> us per iteration
print("frames", B, "wall us/iter (4 GN steps incl. launches):", dt / (4 * L) * 1e6, fs.stats())
fl = out[:, 7][used]
print("of", int(used.sum()), "workgroups:", int((fl & 1).astype(bool).sum()), "in a group on one XCD,", int((fl & 4).astype(bool).sum()), "in a group with two-level sums,", int((fl & 2).astype(bool).sum()), "keep their z in L2 (plain stores)")
print("workgroups active", used.sum(), "tiles/WG", o[used, 5].min(), o[used, 5].max(), "halo cells", (out[:, 6][used] & 0xffffffff).min(), (out[:, 6][used] & 0xffffffff).max())
for n, col in zip(["phaseA", "wait1", "phaseB", "wait2", "update"], us.T):
    print("%-14s mean %.2f  min %.2f  max %.2f us" % (n, col.mean(), col.min(), col.max()))
print("sum of means %.2f us" % us.mean(0).sum())
# inside the two group sums of an iteration (wave 0, shader clocks -> us at the clock the launch ran at, from the stamps)
clk = o[used, 8:12] / (2.0 * L * 4)           # per sum; 4 launches... (the table holds the LAST launch only: / L)
clk = o[used, 8:12] / (2.0 * L)
print("per group sum, shader clocks: block sum %.0f  publish %.0f  poll %.0f  tail %.0f   sweeps per sum %.2f" % (
    clk[:, 0].mean(), clk[:, 1].mean(), clk[:, 2].mean(), clk[:, 3].mean(), (o[used, 12] / (2.0 * L)).mean()))
if o[used, 5].max() >= 9:       # (arap_resident.h: PUBMASK is off in k_pcg_resident<true, 9, RES_SUMS_FLAT>, which has no VGPR for it)
    print("note: a flat launch of the instrumented 9-slot kernel publishes behind a branch on `fast`, production under lane masks:"
          " its `publish` clocks are not production's")
print("repeated looks at the neighbours' z tags per iteration (wave 0 of each workgroup): mean %.3f  max %.3f" % (
    (o[used, 13] / float(L)).mean(), (o[used, 13] / float(L)).max()))
# per-workgroup view of one group (the workgroups of XCD 0: blockIdx & 7 == 0), sorted by tiles then phase A time
idx = np.arange(512)
g0 = used & ((idx & 7) == 0)
rows = sorted(zip(o[g0, 5], (out[:, 6] & 0xffffffff).astype(np.float64)[g0], *(o[g0, c] * 0.01 / L for c in range(5)), idx[g0] >> 3), key=lambda r: (r[0], r[2]))
print("XCD 0 workgroups: tiles halo | phaseA wait1 phaseB wait2 update | local index")
for r in rows:
    print("%3d %5d | %5.2f %5.2f %5.2f %5.2f %5.2f | %2d" % (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]))

# ---- second table (ArapFlow_SolverStampParts): the on-chip chain at both ends of a group sum, and who arrives last ----
q = np.zeros((512, 16), np.uint64)
assert st.lib.ArapFlow_SolverStampParts(fs.h, q.ctypes.data) == 0
qf = q.astype(np.float64)
one = used & ((out[:, 7] & 4) == 0)         # the split clocks are taken in group_sum (groups on one XCD) only
per = qf[one] / (2.0 * L)                     # per sum: both sums of every iteration are summed
print("per group sum, shader clocks (wave 0, mean over %d workgroups):" % int(one.sum()))
print("  entry: wave tree %.0f | LDS + barrier %.0f | final level %.0f    exit: lane tree %.0f | broadcast (barrier + read) %.0f" % (
    per[:, 0].mean(), per[:, 1].mean(), per[:, 2].mean(), per[:, 3].mean(), per[:, 4].mean()))
print("  (LDS + barrier includes the wait for the workgroup's slowest wavefront; each part includes one s_memtime)")
# arrival: mean publish time of a workgroup over the launch's iterations, against its group's mean (100 MHz -> us)
rank = (q[:, 11] & 0xffff).astype(np.int64)
wgs = ((q[:, 11] >> 16) & 0xffff).astype(np.int64)
slot = (q[:, 11] >> 32).astype(np.int64)
tiles, halo, exg = qf[:, 8], qf[:, 9], qf[:, 10]
hw = q[:, 7]
cukey = ((hw >> 32) << 16) | ((hw >> 8) & 0xff)          # XCC id, SE / SH / CU of HW_ID
first = np.zeros(512, bool)                               # the CU's first workgroup (lower blockIdx) of the two it holds
for k in np.unique(cukey[used]):
    m = np.flatnonzero(used & (cukey == k))
    first[m.min()] = True
arr = np.zeros((512, 2))
for g in np.unique(slot[used]):
    m = used & (slot == g)
    for s_ in range(2):
        t = (q[m, 5 + s_] - q[m, 5 + s_].min()).astype(np.float64) / L      # (integer difference first: the sums are ~1e15)
        arr[m, s_] = (t - t.mean()) * 0.01
am = arr[used]
print("arrival at the group sums, us after the group's mean arrival (mean over the iterations), all workgroups:")
for s_, nm in enumerate(["sum 1 (sigma)", "sum 2 (rho)"]):
    print("  %-14s min %+.3f  p25 %+.3f  median %+.3f  p75 %+.3f  max %+.3f   spread per group (max - min): mean %.3f" % (
        (nm,) + tuple(np.percentile(am[:, s_], [0, 25, 50, 75, 100])) +
        (np.mean([np.ptp(arr[used & (slot == g), s_]) for g in np.unique(slot[used])]),)))
def corr(a, b):
    return float(np.corrcoef(a, b)[0, 1]) if a.std() > 0 and b.std() > 0 else float("nan")
for s_, nm in enumerate(["sum 1", "sum 2"]):
    print("  %s: correlation of the arrival with tiles %+.2f, halo cells %+.2f, export granules %+.2f, first of its CU %+.2f;"
          " mean arrival of the CU's first / second workgroup %+.3f / %+.3f us" % (
              nm, corr(am[:, s_], tiles[used]), corr(am[:, s_], halo[used]), corr(am[:, s_], exg[used]),
              corr(am[:, s_], first[used].astype(float)), arr[used & first, s_].mean(), arr[used & ~first, s_].mean()))
g0 = slot[used].min()
m = np.flatnonzero(used & (slot == g0))
print("group of batch slot %d (%d workgroups), sorted by arrival at sum 1: rank tiles halo export CU-mate | arrival sum 1 / sum 2 (us)" % (g0, len(m)))
for i in m[np.argsort(arr[m, 0])]:
    print("  %3d %3d %4d %4d %-6s | %+.3f %+.3f" % (rank[i], tiles[i], halo[i], exg[i], "first" if first[i] else "second",
                                                  arr[i, 0], arr[i, 1]))
