"""from a rocprofv3 kernel trace (csv): how much of every k_score_many dispatch's interval lies inside a k_score_fast dispatch's"""
import csv, glob, sys
d = sys.argv[1]
paths = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
rows = []
for p in paths:
    with open(p) as f:
        for r in csv.DictReader(f):
            rows.append(r)
def name(r): return r.get("Kernel_Name") or r.get("KernelName") or ""
def t(r, k): return int(r[k])
fast = [(t(r, "Start_Timestamp"), t(r, "End_Timestamp")) for r in rows if "k_score_fast" in name(r)]
many = [(t(r, "Start_Timestamp"), t(r, "End_Timestamp"), r.get("Grid_Size_X") or r.get("Grid_Size") or "?") for r in rows if "k_score_many" in name(r)]
print("trace files", paths, "dispatches", len(rows), "k_score_fast", len(fast), "k_score_many", len(many))
for s, e, g in sorted(many):
    inside = sum(max(0, min(e, fe) - max(s, fs)) for fs, fe in fast)
    near = min(fast, key=lambda x: abs(x[0] - s)) if fast else (0, 0)
    print(f"k_score_many grid {g}: {(e - s) / 1e6:.3f} ms, inside k_score_fast {inside / 1e6:.3f} ms ({100.0 * inside / max(1, e - s):.1f} %); that k_score_fast: {(near[1] - near[0]) / 1e6:.3f} ms, starts {(near[0] - s) / 1e6:+.3f} ms after it")
