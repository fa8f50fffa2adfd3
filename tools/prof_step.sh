#!/bin/bash
# rocprofv3 kernel trace of bench.py and one steady-state step's timeline: bash tools/prof_step.sh <tag> [bench args]
tag=$1; shift
root=$(pwd)
out=${OUT_DIR:-bench_out}; mkdir -p "$out"; out=$(cd "$out" && pwd)      # where results go (OUT_DIR=<dir> to choose)
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/prof_${tag} -o ${tag} -- python3 $root/bench.py --full --no-cpu-baseline --steps 20 --warmup 10 --repeats 2 "$@" > $out/prof_${tag}.json 2> $out/prof_${tag}.err
echo "prof rc=$?"
cd $root
python3 tools/step_timeline.py $out/prof_${tag}/${tag}_results.db | tee $out/${tag}_timeline.txt
