# kernel-trace statistics of the bench command (1 step + 1 warm-up), round 2
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
# --full: the statistics include the k_pbs_wide rows of the single_block leg (profiles/README.md, r02);  usage: prof_bench_r02.sh OUT_DIR
O="${1:?output directory}"
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O -o bench -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-other-modes > $O.log 2>&1 &&
head -12 $O/*kernel_stats.csv | cut -c1-300
