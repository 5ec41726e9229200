"""Per replay (the last 20 graph replays of tools/graph_probe.py under rocprofv3 --kernel-trace): launches, kernel time and the time
alone of the OccHead coarse-stage tail chains (pred: the first launches after the mix kernel; soft: the last before it), each with
the means of three groups of replays:
    python tools/graph_chain.py DIR/gp_kernel_trace.csv"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "")
idx = [i for i, r in enumerate(rows) if "k_occhead_mix" in name(r)]
n = 20
reps = [rows[idx[-n - 1 + j] + 1: idx[-n + j] + 1] for j in range(n)]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
def stats(v):
    g = [sum(v[0:7]) / 7, sum(v[7:14]) / 7, sum(v[14:20]) / 6]
    return "mean %.1f us  min %.1f  max %.1f | means of replays 1-7 / 8-14 / 15-20: %.1f %.1f %.1f" % (sum(v) / len(v), min(v), max(v), g[0], g[1], g[2])
print("launches per replay:", sorted(set(len(r) for r in reps)))
print("kernel time per replay:", stats([sum(dur(k) for k in r) for r in reps]))
# a replay (shifted) starts right after the mix kernel: the pred chain is its first launches, the soft chain its last before the mix
def chain(r, lo, hi):
    return sum(dur(k) for k in r[lo:hi]), [name(k)[:28] for k in r[lo:hi]]
last = reps[-1]
fused = "k_head_pred_h2" in name(last[0])
npred, nsoft = (1, 1) if fused else (4, 2)
print("pred chain:", chain(last, 0, npred)[1], stats([chain(r, 0, npred)[0] for r in reps]))
print("soft chain:", chain(last, len(last) - 1 - nsoft, len(last) - 1)[1], stats([chain(r, len(r) - 1 - nsoft, len(r) - 1)[0] for r in reps]))
