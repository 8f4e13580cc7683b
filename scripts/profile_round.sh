#!/bin/bash
# Regenerates the round's artefacts under $OUT (default profile_out/; copy the ones to keep into profiles/):
#   bench line (N = 1, --full), rocprofv3 --kernel-trace --stats of the same command, MFMA / wave-state / LDS counters,
#   conv / gemm / front-end micro-benchmarks, training benchmark, in-kernel stamps of the conv kernel (diagnostic build).
set -e
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-$R/profile_out}     # results folder (OUT=<dir> to change it)
export OUT
mkdir -p "$OUT"
TAG=${1:-r02}
cd $R
python3 bench.py --full > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}_bench.err"
echo bench done
cd /tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${TAG}_stats" -- python3 $R/bench.py --full --no-cpu-baseline --no-small-batch --no-parity-mode --no-h2d --no-train-leg > "$OUT/${TAG}_bench_profiled.json" 2>/dev/null
echo stats done
cd $R
bash scripts/profile_mfma_counters.sh ${TAG}
python3 scripts/conv_bench.py 10240 bf16 > "$OUT/${TAG}_conv_bench.txt" 2>/dev/null
python3 scripts/conv_bench.py 10240 f32 5 >> "$OUT/${TAG}_conv_bench.txt" 2>/dev/null
python3 scripts/gemm_bench.py 10240 bf16 > "$OUT/${TAG}_gemm_bench.txt" 2>/dev/null
python3 scripts/gemm_bench.py 10240 f32 >> "$OUT/${TAG}_gemm_bench.txt" 2>/dev/null
python3 scripts/fe_bench.py > "$OUT/${TAG}_fe_bench.txt" 2>/dev/null
python3 scripts/train_bench.py > "$OUT/${TAG}_train_bench.txt" 2>/dev/null
python3 scripts/wgrad_bench.py > "$OUT/${TAG}_wgrad_bench.txt" 2>/dev/null
echo all done
