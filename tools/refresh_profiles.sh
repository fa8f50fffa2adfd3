#!/bin/bash
# Regenerate the round's measurement artifacts ON the GPU box (from the repository root):
#   bash tools/refresh_profiles.sh r01        -> bench_out/<tag>_* or OUT_DIR/<tag>_*  (copy the ones to keep into profiles/)
set -e -o pipefail
tag=${1:-r01}
root=$(pwd)
out=${OUT_DIR:-bench_out}; mkdir -p "$out"; out=$(cd "$out" && pwd)      # where results go (OUT_DIR=<dir> to choose)
timeout -k 10 400 python3 bench.py --full > $out/${tag}_bench_wide.json 2> $out/${tag}_bench.err
timeout -k 10 300 python3 bench.py --full --config small > $out/${tag}_bench_small.json 2>> $out/${tag}_bench.err
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/prof_${tag} -o ${tag} -- python3 $root/bench.py --full --no-cpu-baseline --steps 20 --warmup 10 > /dev/null 2>&1 || true
cd $root
python3 profiles/summarize_db.py $out/prof_${tag}/${tag}_results.db 30 > $out/${tag}_wide_kernel_stats.txt
OUT_DIR=$out timeout -k 10 900 python3 tools/collect_traffic.py ${tag} > $out/${tag}_traffic.log 2>&1
tail -4 $out/${tag}_traffic.log
