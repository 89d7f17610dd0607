# the final bench lines of a round: bash tools/lab/final_bench.sh OUTDIR
O=${1:?usage: bash tools/lab/final_bench.sh OUTDIR}
cd $GRAFT_REPO_ROOT
mkdir -p "$O"
timeout -k 10 600 python bench.py --full > "$O/bench.json" 2> "$O/bench.err"
timeout -k 10 300 python bench.py --force-dist --no-cpu --no-micro --no-long-run --no-mpm > "$O/bench_force_dist.json" 2> /dev/null
timeout -k 10 300 python bench.py --no-cpu --no-micro --no-long-run --no-mpm > "$O/bench_single_same_run.json" 2> /dev/null
