#!/bin/bash
# GPU: kernel timeline of ONE evaluation at a small size (default N = 4096 = BASELINE configs[1]) from a rocprofv3 kernel trace
#   bash tools/c2_trace.sh OUTDIR [N] [TRACEDIR]      (TRACEDIR: where rocprofv3 writes the raw trace; default: a fresh mktemp -d)
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "$1" && cd "$1" && pwd); N=${2:-4096}; T=${3:-$(mktemp -d)}
rm -rf "$T"; timeout 300 rocprofv3 --output-format csv --kernel-trace -d "$T" -o run -- python $R/bench.py --n $N --d 8 --kind rbf --iso --steps 40 --warmup 10 --full --no-legs --no-cpu-baseline --no-parity-gate > $O/trace_bench_$N.json 2> $O/trace_prof_$N.err
f=$(find "$T" -name "run_kernel_trace.csv" | head -1); for b in 8 20; do python $R/tools/eval_timeline.py $f $b; done > $O/timeline_$N.txt
