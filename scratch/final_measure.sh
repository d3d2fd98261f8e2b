#!/bin/bash
# usage: scratch/final_measure.sh <tag> [output dir, default measure_out]   -- the round's measurement set on ONE box: full bench line,
# interleaved A/B against the previous round's tree, bench under rocprofv3 (kernel stats, category summary, kernel sequence), matrix-pipe
# busy share per kernel, HBM traffic per kernel
tag=${1:-r05_v1}
out=${2:-measure_out}; mkdir -p $out
python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
echo "bench: $(cut -c1-220 $out/${tag}_bench.json)"
bash scratch/ab_base.sh 3 100 > $out/${tag}_ab_vs_previous_round.txt 2>&1
cat $out/${tag}_ab_vs_previous_round.txt
bash scratch/measure.sh $tag $out > $out/${tag}_meas.txt 2>&1
head -20 $out/cat_$tag.txt
bash scratch/pmc_mfma.sh > $out/${tag}_mfma_busy_per_kernel.txt 2>&1
head -12 $out/${tag}_mfma_busy_per_kernel.txt
bash scratch/pmc_bench_traffic.sh $PWD/$out/${tag}_traffic.json > $out/${tag}_traffic_top.txt 2>&1
head -5 $out/${tag}_traffic_top.txt
