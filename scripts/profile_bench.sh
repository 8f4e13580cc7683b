#!/bin/bash
# round-1 recipe: bench line + rocprofv3 --kernel-trace --stats of the same command (round 2: scripts/profile_round.sh); results under $OUT
set -e
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/profile_out}     # results folder (OUT=<dir> to change it)
mkdir -p "$OUT"
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/bench_stats2" -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-small-batch > "$OUT/bench_prof_line.json" 2>/dev/null
cd $R
python3 bench.py --full --steps 10 --warmup 3 2>/dev/null | tail -1 > "$OUT/bench_line.json"
python3 scripts/fe_bench.py > "$OUT/fe_bench.txt" 2>/dev/null
python3 scripts/conv_bench.py 10240 bf16 > "$OUT/conv_bench.txt" 2>/dev/null
python3 scripts/conv_bench.py 10240 f32 5 >> "$OUT/conv_bench.txt" 2>/dev/null
python3 scripts/gemm_bench.py 10240 bf16 > "$OUT/gemm_bench.txt" 2>/dev/null
python3 scripts/gemm_bench.py 10240 f32 >> "$OUT/gemm_bench.txt" 2>/dev/null
python3 scripts/train_bench.py > "$OUT/train_bench.txt" 2>/dev/null
echo done
