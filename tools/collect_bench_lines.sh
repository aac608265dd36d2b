#!/bin/bash
# Runs bench.py --full for every workload on the local GPU and writes the JSON lines to <dir>/<workload>.json
# (tools/merge_bench_lines.py <tag> <dir> folds them into profiles/<tag>_bench_lines.json).  Developer tool.  usage: tools/collect_bench_lines.sh <dir>
set -e
mkdir -p "${1:?usage: tools/collect_bench_lines.sh <dir>}"
out=$(cd "$1" && pwd)
cd "$(dirname "$0")/.."
timeout -k 10 900 python3 bench.py --full > $out/cfg5.json 2> $out/cfg5.err
timeout -k 10 600 python3 bench.py --full --labeling degree --no-cpu > $out/cfg5_degree.json 2> /dev/null
timeout -k 10 600 python3 bench.py --full --workload cfg5n > $out/cfg5n.json 2> /dev/null
for w in cfg4 cfg3 cfg2 hcp148; do
  timeout -k 10 300 python3 bench.py --full --workload $w --steps 100 --warmup 20 > $out/$w.json 2> /dev/null
done
timeout -k 10 300 python3 tools/train_bench.py > $out/train_dx.txt 2> /dev/null
timeout -k 10 300 python3 tools/train_bench.py --no-dx > $out/train_nodx.txt 2> /dev/null
echo done
