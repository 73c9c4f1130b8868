#!/usr/bin/env python3
"""Per-kernel average duration of two rocprofv3 --stats csv files side by side: stats_diff.py before.csv after.csv [N rows]."""
import csv
import sys


def load(path):
    with open(path, newline="") as f:
        return {r["Name"]: r for r in csv.DictReader(f)}


def short(name):
    return name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]


a, b = load(sys.argv[1]), load(sys.argv[2])
top = int(sys.argv[3]) if len(sys.argv) > 3 else 24
ta = sum(float(r["TotalDurationNs"]) for r in a.values())
tb = sum(float(r["TotalDurationNs"]) for r in b.values())
print("kernel | calls | share before % | average before us | average after us | after / before")
for name in sorted(a, key=lambda n: -float(a[n]["TotalDurationNs"]))[:top]:
    ra, rb = a[name], b.get(name)
    if rb is None:
        continue
    ua, ub = float(ra["AverageNs"]) / 1e3, float(rb["AverageNs"]) / 1e3
    print(f"{short(name)} | {ra['Calls']} | {float(ra['Percentage']):.2f} | {ua:.1f} | {ub:.1f} | {ub / ua:.4f}")
print(f"all kernels, total duration ms | | | {ta / 1e6:.1f} | {tb / 1e6:.1f} | {tb / ta:.4f}")
