#!/usr/bin/env python3
"""<dir>/*.json (tools/collect_bench_lines.sh <dir>) -> profiles/<tag>_bench_lines.json.  Developer tool.  usage: merge_bench_lines.py <tag> <dir>"""
import glob
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if len(sys.argv) != 3:
    sys.exit("usage: tools/merge_bench_lines.py <tag> <dir>")
tag, src = sys.argv[1], sys.argv[2]
out = {}
for f in sorted(glob.glob(os.path.join(src, "*.json"))):
    lines = [l for l in open(f).read().splitlines() if l.startswith("{")]
    if lines:
        out[os.path.basename(f)[:-5]] = json.loads(lines[-1])
for f in sorted(glob.glob(os.path.join(src, "train_*.txt"))):
    out[os.path.basename(f)[:-4]] = [l for l in open(f).read().splitlines() if "forward" in l or "HCP-style" in l]
json.dump(out, open(os.path.join(ROOT, "profiles", tag + "_bench_lines.json"), "w"), indent=1)
for k, v in out.items():
    if isinstance(v, dict):
        print(k, v["value"], v["ms_per_step"], (v.get("roofline") or {}).get("frac"), (v.get("cpu_baseline") or {}).get("value"))
    else:
        print(k, *v, sep="\n   ")
