#!/bin/bash
# Batches in flight (--streams) A/B on one box.
# Output under $OUT_DIR (default bench_out/).
set -o pipefail
O=${OUT_DIR:-bench_out}
mkdir -p $O
for s in ${STREAMS:-1 2 3}; do
  timeout -k 10 300 python bench.py --full --steps 30 --warmup 5 --streams $s --no-cpu-baseline --no-peak-run --no-adversarial --c3-requests 0 --no-extra-lines > $O/streams_ab_$s$SUF.json 2> $O/streams_ab_$s$SUF.err || exit 1
  python3 -c "import json;d=json.load(open('$O/streams_ab_$s$SUF.json'));print('$s$SUF', d['ms_per_step'], d['kernel_ms'])"
done
