# rocprofv3 kernel-trace summary of the bench command with all its legs (profiles/r01_bench_kernel_stats.csv)
# usage: tools/prof_bench.sh OUTPUT_DIR   (an absolute path: the profiler runs from /tmp)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
OUT=${1:?usage: tools/prof_bench.sh OUTPUT_DIR}
mkdir -p $OUT
rocprofv3 --kernel-trace --stats -f csv -d $OUT -o bench -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/bench_under_rocprof.json 2> $OUT/err.log
ls $OUT
tail -c 400 $OUT/bench_under_rocprof.json
