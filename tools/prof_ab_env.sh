#!/bin/bash
# kernel-trace timeline of one wide step per setting of an environment switch (lab): tools/prof_ab_env.sh VAR v1 v2 ...
root=$(pwd); var=$1; shift
out=${OUT_DIR:-bench_out}; mkdir -p "$out"; out=$(cd "$out" && pwd)      # where results go (OUT_DIR=<dir> to choose)
for v in "$@"; do
  export $var=$v
  (cd /tmp && export TMPDIR=/tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/prof_ab_$v -o ab -- python3 $root/bench.py --full --no-cpu-baseline --no-reporting-config --no-deep-config --no-train-step --no-box --steps 20 --warmup 10 --repeats 2 > /dev/null 2>&1; echo "prof $var=$v rc=$?")
  python3 tools/step_timeline.py $out/prof_ab_$v/ab_results.db > $out/ab_${var}_$v.txt 2>&1; cat $out/ab_${var}_$v.txt
done
