#!/bin/bash
# Clock / power under sustained verify load: a long bench run (2,000 steps
# of 1M verifies) in the background while amd-smi samples the GPU's power
# and clocks every ~0.3 s; then the same for synchronized single batches.
# Output under $OUT_DIR (default bench_out/) in the repository.
cd "$(dirname "$0")/.." || exit 1
O=${OUT_DIR:-bench_out}/clk
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 python bench.py --full --steps 2000 --warmup 5 --latency-reps 3 --no-cpu-baseline --no-peak-run \
  > $O/bench_long.json 2> $O/bench_long.err &
pid=$!
for k in $(seq 1 200); do
  kill -0 $pid 2>/dev/null || break
  { echo "T $(date +%s.%N)"; timeout 5 amd-smi metric -g 0 -p -c 2>&1; timeout 5 rocm-smi -d 0 --showpower --showclocks 2>&1; } >> $O/samples.txt
  sleep 0.3
done
wait $pid
echo "bench rc=$?"
python3 -c "import json;d=json.load(open('$O/bench_long.json'));print('long value %.1fM ms/step %.4f k_verify %.4f'%(d['value']/1e6,d['ms_per_step'],d['kernel_ms']['k_verify']))"
