#!/bin/bash
# usage: scratch/measure.sh <tag> [output dir, default measure_out]   -- bench under rocprofv3 kernel trace, category summary per iteration,
# kernel sequence of one iteration
export GANK_BENCH_EXTRAS=0     # bench.py: the headline measurement only (no fp16 child, no other configurations)
tag=${1:-m}
out=${2:-measure_out}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $out && rm -rf $out/prof_$tag
# --full: the 27 iterations below are 5 warm-up + 20 timed + the roofline pass's 2 eager ones
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/prof_$tag -o $tag --output-format csv -- python3 bench.py --full --no-cpu-baseline --steps 20 --warmup 5 > $out/bench_$tag.json 2> $out/bench_$tag.err < /dev/null
python3 scratch/cat_summary.py $out/prof_$tag 27 > $out/cat_$tag.txt 2>&1
grep -o '"value": [0-9.]*\|"ms_per_step": [0-9.]*' $out/bench_$tag.json | head -2
head -14 $out/cat_$tag.txt
python3 scratch/seq_dump.py $out/prof_$tag 1000 > $out/seq_$tag.txt 2>&1
rm -f $out/prof_$tag/*kernel_trace.csv
