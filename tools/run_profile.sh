# Round profile of the bench command (run on the GPU box through gpurun): bench line, rocprofv3 kernel stats, and the two
# PMC passes (FETCH_SIZE / WRITE_SIZE separately, without any trace domain, as the MI355X guide prescribes).
#   R=r02 bash tools/run_profile.sh        -> $OUT = profile_out/$R/{bench.json,stats/,stats_overlap/,traffic.json}
# Every bench line is a `bench.py --full` line: the profile set records `roofline`, `alt_arith` and the kernels of both runs.
# The kernel-stats pass that bench.py's rocprof_avg_us reads runs with BDVCIL_WGRAD_SIDE_STREAM=0: with the weight gradients on
# their own stream (the default) two kernels share the GPU and every duration in the trace is stretched by its neighbour; the
# same pass with the default streams is kept beside it (stats_overlap).
set -e
R=${R:-r02}
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
OUT=${OUT:-profile_out/$R}
rm -rf "$OUT"
mkdir -p "$OUT"
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err
BDVCIL_WGRAD_SIDE_STREAM=0 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/stats_bench.json 2> $OUT/stats.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_overlap -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/stats_overlap_bench.json 2> $OUT/stats_overlap.err
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing > $OUT/pmc_fetch.json 2> $OUT/pmc_fetch.err
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing > $OUT/pmc_write.json 2> $OUT/pmc_write.err
python tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write > $OUT/traffic.json
# the other workloads of BASELINE.json (not the metric)
timeout -k 10 300 python bench.py --full --workload cil --steps 8 --warmup 2 --no-cpu-baseline > $OUT/bench_cil.json 2> $OUT/bench_cil.err
timeout -k 10 300 python bench.py --full --workload predict --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_predict.json 2> $OUT/bench_predict.err
timeout -k 10 300 python bench.py --full --workload i3d --steps 8 --warmup 2 --no-cpu-baseline > $OUT/bench_i3d.json 2> $OUT/bench_i3d.err
timeout -k 10 300 python bench.py --full --arith bf16x2 --no-cpu-baseline > $OUT/bench_bf16x2.json 2> $OUT/bench_bf16x2.err
timeout -k 10 300 python bench.py --full --arith bf16x1 --batch 64 --steps 8 --warmup 3 --no-cpu-baseline > $OUT/bench_bf16x1.json 2> $OUT/bench_bf16x1.err
timeout -k 10 300 python bench.py --full --arith bf16 --batch 64 --no-cpu-baseline > $OUT/bench_bf16.json 2> $OUT/bench_bf16.err
timeout -k 10 300 python bench.py --full --arith bf16 --workload cil --steps 8 --warmup 2 --no-cpu-baseline > $OUT/bench_cil_bf16.json 2> $OUT/bench_cil_bf16.err
timeout -k 10 300 python bench.py --full --arith bf16 --workload predict --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_predict_bf16.json 2> $OUT/bench_predict_bf16.err
timeout -k 10 300 python bench.py --full --depth 34 --no-cpu-baseline > $OUT/bench_r34.json 2> $OUT/bench_r34.err
timeout -k 10 300 python bench.py --full --arith f32mfma --no-cpu-baseline > $OUT/bench_f32mfma.json 2> $OUT/bench_f32mfma.err
find $OUT -name "*counter_collection.csv" -size +8M -delete
find $OUT -name "*kernel_trace.csv" -delete
ls -la $OUT $OUT/stats/* | head -40
